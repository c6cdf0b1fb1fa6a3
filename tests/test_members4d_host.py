"""Host checks of the ensembles of 4-D members (`odil.util.optimize_ensemble` for fields on (t, x, y, z):
examples/velocity_from_tracer/veltracer3d.py), no GPU -- everything here is answered from shapes, or traced on CPU tensors:

1  odil_mg_members_levels_ok admits the layouts tests/test_members4d_gpu.py runs, in both element sizes, and keeps its
   limit on the rows; the levels of those layouts run the three transposes the row variants exist for
2  `fused.traced_refusal` admits 4-D level shapes under form 'volumes' and names the form under 'launches';
   `ensemble._traced_form` takes 'volumes' for them
3  the refusals that stay name the member and leave the states alone, before any operator is traced
4  the generator emits the batched kernels of veltracer3d with the bodies of the single ones, also for float32 members
   with a last axis of 128 cells (no network: no marching forward kernel); a 4-D member WITH a network and such an axis
   marches, and the generator refuses its batched form
5  a 2-D member with one cell-centred unknown still reports `stacked == False`"""

import argparse

import numpy as np
import pytest
import torch
from fields_ensemble_members import pair_operator, randomise, run_args
from members4d import FAST, LAYOUT_IDS, LAYOUTS4, NODE, TRACER3D_LEVELS, cell4, kinds_of, net4, tracer3d
from test_traced_ensemble_host import body_after_head, cpu_mod, generate, kernel_lines, snapshot, unchanged  # noqa: F401

import odil_amd as odil
from odil_amd import _lib, ensemble, fused, stencil_jit
from odil_amd.stencil_trace import TraceUnsupported


def levels_ok(loc, shapes, nrows, elem_size):
    lib = _lib.load()
    flat = [int(n) for s in shapes for n in s]
    code = lib.odil_mg_members_levels_ok(_lib.i64(flat), len(shapes), len(shapes[0]), loc.encode(), nrows, elem_size)
    return code, lib.odil_last_error().decode()


# --------------------------------------------------------------------------------------------------------- 1: the library
@pytest.mark.parametrize("elem_size", [8, 4], ids=["f64", "f32"])
@pytest.mark.parametrize("loc,shapes,kinds", LAYOUTS4, ids=LAYOUT_IDS)
def test_library_admits_the_rows_of_the_gpu_layouts(loc, shapes, kinds, elem_size):
    assert levels_ok(loc, shapes, 6, elem_size)[0] == 0
    assert levels_ok(loc, shapes, 65535, elem_size)[0] == 0
    code, text = levels_ok(loc, shapes, 70000, elem_size)
    assert code != 0 and "70000 rows" in text
    assert kinds_of(_lib.load(), _lib.i64, loc, shapes, elem_size) == kinds


@pytest.mark.parametrize("elem_size", [8, 4], ids=["f64", "f32"])
def test_kinds_of_single_4d_levels(elem_size):
    """What the row variants were built for: a single 4-D level runs the node-centred marching kernel ('nccc' with four
    coarse x-planes or more), the fast kernel (last two axes cell-centred) or the generic one (a node-centred y or x
    axis) -- never the rows, tile or all-cell marching kernels."""
    lib = _lib.load()
    kind = lambda loc, cshape: lib.odil_interp_adj_kind(_lib.i64(list(cshape)), 4, loc.encode(), elem_size)
    for cshape in [(3, 4, 4, 4), (2, 4, 4, 4), (3, 8, 8, 8), (5, 16, 16, 32)]:
        assert kind("nccc", cshape) == 2, cshape
    for cshape in [(2, 2, 2, 2), (2, 2, 2, 8), (3, 3, 64, 64)]:
        assert kind("nccc", cshape) == 1, cshape
    for loc in ("cccc", "cncc", "nncc"):
        for cshape in [(2, 2, 2, 2), (4, 4, 4, 4), (3, 8, 8, 8), (4, 16, 64, 64)]:
            assert kind(loc, cshape) == 1, (loc, cshape)
    for loc in ("cccn", "ccnc", "nnnn"):
        for cshape in [(2, 2, 2, 2), (2, 2, 3, 2), (4, 8, 8, 8)]:
            assert kind(loc, cshape) == 0, (loc, cshape)


def test_library_keeps_its_limits_for_4d_rows():
    code, text = levels_ok("nccc", [(5, 8, 8, 8), (3, 4, 4, 5)], 4, 8)
    assert code != 0 and "does not refine" in text
    code, text = levels_ok("nccc", [(5, 8, 8, 8)], 4, 8)
    assert code != 0 and "nlvl=1" in text
    code, text = levels_ok(".ccc", [(5, 8, 8, 8), (5, 4, 4, 4)], 4, 8)
    assert code != 0 and "every axis of a row is 'c' or 'n'" in text
    # 2^31 elements in level 1 of a row: named with its level
    code, text = levels_ok("cccc", [(128, 256, 256, 512), (64, 128, 128, 256), (32, 64, 64, 128)], 2, 4)
    assert code != 0 and "level 1 of a row has 2^31 elements or more" in text
    # generic rows are read by the element: 81 elements per row are admitted
    assert levels_ok("nnnn", [(3, 3, 3, 3), (2, 2, 2, 2)], 5, 8)[0] == 0
    assert levels_ok("nccc", [(3, 4, 2, 2), (2, 2, 1, 1)], 5, 4)[0] != 0  # (an extent of 1 on a refined axis)
    # coarse rows of the fast kind can be odd: 3^4 = 81 elements are no multiple of 16 bytes in either element size (a
    # single run of such a member packs its later arrays off the 16-byte grid the members' rows lie on)
    for elem_size in (8, 4):
        code, text = levels_ok("cccc", [(6, 6, 6, 6), (3, 3, 3, 3)], 4, elem_size)
        assert code != 0 and "level 1 of 4 rows" in text and "16-byte grid" in text
    assert levels_ok("cccc", [(12, 12, 12, 12), (6, 6, 6, 6)], 4, 4)[0] == 0


# ------------------------------------------------------------------------------------------------- 2: traced_refusal, form
def test_traced_refusal_admits_4d_members_under_volumes():
    f64, f32 = torch.float64, torch.float32
    nccc = [(5, 8, 8, 8), (3, 4, 4, 4), (2, 2, 2, 2)]
    for dtype in (f64, f32):
        assert fused.traced_refusal(nccc, dtype, "volumes", 5, loc="nccc", nfields=4) is None
        assert fused.traced_refusal([(8, 8, 8, 8), (4, 4, 4, 4)], dtype, "volumes", 3, loc="cccc", nfields=1) is None
        assert fused.traced_refusal([(8, 8, 8, 8), (4, 4, 4, 4)], dtype, "volumes", 3) is None  # (loc not given: all cells)
        assert fused.traced_refusal([(5, 8, 8, 8)], dtype, "volumes", 3, loc="nccc", nfields=4) is None  # plain Fields
        assert fused.traced_refusal([(4, 4, 4, 5), (2, 2, 2, 3)], dtype, "volumes", 2, loc="cccn", nfields=2) is None
        reason = fused.traced_refusal(nccc, dtype, "launches", 5, loc="nccc", nfields=4)
        assert "4-D grid: form 'launches' runs 1-D and 2-D grids" in reason
        assert "form 'launches'" in fused.traced_refusal([(8, 8, 8, 8), (4, 4, 4, 4)], dtype, "launches", 3)
    assert "rows (1 ... 65535)" in fused.traced_refusal(nccc, f64, "volumes", 20000, loc="nccc", nfields=4)
    assert "5-D" in fused.traced_refusal([(4,) * 5], f64, "volumes", 2, loc="ccccc")
    # fully node-centred float64 members of 81 elements lie back to back off the 16-byte grid, as in 1-D to 3-D
    assert "not a multiple of 16 bytes" in fused.traced_refusal([(3, 3, 3, 3), (2, 2, 2, 2)], f64, "volumes", 2, loc="nnnn")
    # 3-D members keep their answers
    assert fused.traced_refusal([(5, 8, 16), (3, 4, 8)], f32, "volumes", 5, loc="ncc", nfields=3) is None
    assert "3-D" in fused.traced_refusal([(5, 8, 16), (3, 4, 8)], f64, "launches", 5, loc="ncc", nfields=3)


def test_auto_takes_volumes_for_three_dimensions_and_more():
    assert ensemble._traced_form("auto", [(5, 8, 8, 8)]) == "volumes"
    assert ensemble._traced_form("auto", [(5, 8, 8)]) == "volumes"
    assert ensemble._traced_form("auto", [(9, 16)]) == "launches"
    assert ensemble._traced_form("launches", [(5, 8, 8, 8)]) == "launches"


# --------------------------------------------------------------------------------------------- 3: the refusals that stay
def node4(dtype, b, nlvl=2, cells=(4, 4, 4, 8), loc="nccc", locs=None, before=0, **domain_kw):
    """Two coupled fields u, w at 'nccc' on a 4-D grid (`fields_ensemble_members.pair_operator`); locs: another location
    per field; before: elements of an `Array` that stands in front of them; domain_kw: mg_factors, mg_axes."""
    domain = odil.Domain(cshape=list(cells), dimnames=["t", "x", "y", "z"], multigrid=nlvl is not None, mg_nlvl=nlvl, dtype=dtype,
                         **domain_kw)
    rng = np.random.default_rng(77 + b)
    shape = tuple(domain.size(loc=loc))
    extra = argparse.Namespace(c=0.75, f=domain.mod.cast(rng.standard_normal(shape), dtype),
                               q=domain.mod.cast(rng.standard_normal(shape), dtype))
    state = odil.State()
    if before:
        state.fields["coeff"] = odil.Array([0.5] * before)
    for key in ("u", "w"):
        state.fields[key] = odil.Field(None, loc=(locs or dict()).get(key, loc))
    state = domain.init_state(state)
    return randomise(odil.Problem(pair_operator, domain, extra), state, 7000 + b, but=("coeff",))


def test_driver_refuses_4d_members_by_name_before_tracing(cpu_mod, monkeypatch):
    def no_trace(*args, **kwargs):
        raise AssertionError("an operator was traced before the members were checked")

    monkeypatch.setattr(stencil_jit, "trace_outputs", no_trace)
    monkeypatch.setattr(stencil_jit, "trace", no_trace)
    monkeypatch.setattr(fused, "detect", no_trace)
    f64 = np.float64

    def refused(built, match, args=None, driver=None, **kwargs):
        problems, states = [p for p, _ in built], [s for _, s in built]
        before = snapshot(states)
        with pytest.raises(ValueError, match=match):
            (driver or odil.util.optimize_ensemble)(args or run_args(), problems, states, **kwargs)
        assert unchanged(states, before)

    good = lambda b: node4(f64, b)
    # grid unknowns at two locations
    refused([good(0), node4(f64, 1, locs=dict(w="cccc"))],
            "optimize_ensemble: member 1: grid unknowns at two locations: 'u' at 'nccc', 'w' at 'cccc'", form="volumes")
    # multigrid factors other than 1
    refused([good(0), node4(f64, 1, mg_factors=[1.0, 2.0])], r"optimize_ensemble: member 1: multigrid factors \[1.0, 2.0\]",
            form="volumes")
    # multigrid axes that do not all coarsen
    refused([good(0), node4(f64, 1, mg_axes=[False, True, True, True])],
            r"optimize_ensemble: member 1: multigrid axes \[False, True, True, True\]", form="auto")
    # a finest array that is no multiple of 16 bytes: 5^4 = 625 float64 elements
    refused([good(0), node4(f64, 1, cells=(4, 4, 4, 4), loc="nnnn")],
            "optimize_ensemble: member 1: a member of 625 cells is not a multiple of 16 bytes", form="volumes")
    # parameter elements before the first multigrid field that are no multiple of 4: a single run packs its arrays back to
    # back, and its 'nccc' levels then leave the grid of two elements by which the marching transpose is chosen
    refused([good(0), node4(f64, 1, before=3)],
            "optimize_ensemble: member 1: 3 Array elements stand before the 4-D multigrid field", form="volumes")
    # the form of the 1-D / 2-D grids refuses 4-D members by name
    refused([good(0), good(1)], "optimize_ensemble: member 0: 4-D grid: form 'launches' runs 1-D and 2-D grids", form="launches")
    # Newton
    refused([cell4(None, f64, b, cells=(4, 4, 4, 4)) for b in range(2)], "optimize_newton_ensemble: member 0: 4-D grid",
            args=run_args("newton", epochs=2, linsolver="direct"), driver=odil.util.optimize_newton_ensemble)
    refused([good(0), good(1)], "optimize_newton_ensemble: member 0: 2 unknown fields",
            args=run_args("newton", epochs=2, linsolver="direct"), driver=odil.util.optimize_newton_ensemble)


def test_four_elements_before_the_field_are_admitted(cpu_mod):
    """The other side of the rule: a multiple of 4 elements in front leaves a single run's levels where the members' are.
    (On the host the members are then refused for what they are -- the traced kernels need a device -- not for the rule.)"""
    built = [node4(np.float64, b, before=4) for b in range(2)]
    with pytest.raises(ValueError, match="such members run as traced operators"):
        odil.util.optimize_ensemble(run_args(), [p for p, _ in built], [s for _, s in built], form="volumes")


# ------------------------------------------------------------------------------------------------------- 4: generator
@pytest.mark.parametrize("nlvl", [3, None], ids=["3lvl", "plain"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_batched_kernels_of_veltracer3d_share_the_single_bodies(cpu_mod, dtype, nlvl):
    problem, state = tracer3d(nlvl, dtype, 0)
    if nlvl:
        shapes = [tuple(a.shape) for a in problem.domain.arrays_from_field(state.fields["u"])]
        assert shapes == TRACER3D_LEVELS
        for elem_size in (8, 4):
            assert kinds_of(_lib.load(), _lib.i64, "nccc", shapes, elem_size) == [NODE, FAST]
    cg1, single = generate(problem, state, False)
    cg2, batch = generate(problem, state, "params")
    assert "_batch" not in single and "k_fwd_batch" in batch
    assert cg1.gathers == cg2.gathers and cg1.direct == cg2.direct and cg1.merged == cg2.merged
    assert tuple(cg2.G) == (9, 8, 8, 8) and set(cg2.src_keys) == {"u", "vx", "vy", "vz"}
    names = [("k_fwd", "blockIdx.y"), ("k_final", "blockIdx.z"), ("k_loss", "blockIdx.x")]
    names += [("k_gat_all", "blockIdx.y")] if cg2.merged else []
    names += [("k_gat_{}".format(gi), "blockIdx.y") for gi, key in enumerate(cg2.gathers) if key not in cg2.merged]
    for name, member in names:
        one = kernel_lines(single, name)
        assert kernel_lines(batch, name) == one, "{} of the batched source differs".format(name)
        many = kernel_lines(batch, name + "_batch")
        assert body_after_head(many, member) == one[1:], "the bodies of {} differ".format(name)
        assert not any(member in line for line in one)


def test_wide_float_members_of_veltracer3d_do_not_march(cpu_mod):
    """The marching forward kernel (refused in batched form: tests/test_traced_ensemble_host.py) shares the evaluations of
    a pointwise NETWORK between threads -- float32, three or more dimensions, a last axis of 128 cells or more.
    veltracer3d has no network: its float32 members with a last axis of 128 cells generate the plain forward kernel and
    its batched form."""
    cg, source = generate(*tracer3d(None, np.float32, 0, cells=(2, 4, 16, 128)), "params")
    assert cg.share_mode is None and "k_fwd_batch" in source


def test_generator_refuses_the_marching_forward_kernel_of_a_4d_member(cpu_mod):
    """A 4-D member WITH a pointwise network (`net4`): float32 and a last axis of 128 cells make its forward kernel the
    marching one, which has no batched form; float64, and float32 rows of 64 cells, generate the batched kernels."""
    with pytest.raises(TraceUnsupported, match="marching forward kernel"):
        generate(*net4(np.float32, 0), "params")
    assert "k_fwd_batch" in generate(*net4(np.float64, 0), "params")[1]
    assert "k_fwd_batch" in generate(*net4(np.float32, 0, cells=(2, 4, 16, 64)), "params")[1]


# --------------------------------------------------------------------------------------------------------- 5: stacked
def test_one_cell_centred_unknown_below_four_dimensions_is_not_stacked():
    """`TracedLaunchEnsemble.stacked` (`fused.rows_stacked`): one cell-centred 2-D or 3-D unknown keeps the launches it
    always made; every 4-D member takes the stacked rows."""
    assert fused.rows_stacked(1, "cc") is False and fused.rows_stacked(1, "ccc") is False and fused.rows_stacked(1, "c") is False
    assert fused.rows_stacked(2, "cc") is True and fused.rows_stacked(1, "nc") is True
    assert fused.rows_stacked(1, "cccc") is True and fused.rows_stacked(4, "nccc") is True
