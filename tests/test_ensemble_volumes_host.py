"""The ensemble of 3-D Poisson problems as batched launches (odil_poisson_residual_synth_batch,
odil_poisson_adjoint_adam_volumes, odil_mg_synth_adj_adam_members, fused.PoissonVolumeEnsemble,
util.optimize_ensemble(form="volumes")) as far as it can be checked without a device: the library exports the entry points
and header, library and `_lib.EXPORTED` agree; the launchers refuse malformed arguments with an error text before anything
is launched (every pointer is a dummy, so a launch that did happen could not succeed: tests/test_ensemble_launches_host.py
is the model); `optimize_ensemble` names the first member that cannot join, from shapes alone; and the choice between the
forms is a function of shapes and dtype."""

import os
import re
import sys
from ctypes import c_int, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["odil_poisson_residual_synth_batch", "odil_poisson_adjoint_adam_volumes", "odil_mg_synth_adj_adam_members"]
QUERIES = ["odil_mg_members_levels_ok", "odil_interp_adj_kind", "odil_poisson_residual_synth_batch_workspace_bytes",
           "odil_poisson_residual_synth_batch_partials"]


def test_library_header_and_bindings_agree_on_the_new_entry_points():
    from odil_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    declared = set(re.findall(r"\b(odil_\w+)\s*\(", header))
    for name in [n + s for n in NEW for s in ("_f64", "_f32")] + QUERIES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
        assert name in declared, name
    for name in _lib.EXPORTED:
        assert hasattr(lib, name) and name in declared, name
    for name in [n + s for n in NEW for s in ("_f64", "_f32")]:
        assert getattr(lib, name).argtypes, name


def test_a_long_member_has_several_z_chunks_of_column_sums():
    """The per-member workspace of (64, 8, 16): bytes / (8 cny cnx) is the number of z-chunks whose column sums the loss
    replay reduces -- more than one, so the GPU case of this shape does run several chunks per member.  The query is per
    member: the same bytes as the single launch's workspace."""
    from odil_amd import _lib, ops

    lib = _lib.load()
    cshape = (32, 4, 8)
    per_member = lib.odil_poisson_residual_synth_batch_workspace_bytes(_lib.i64(cshape))
    assert per_member == lib.odil_poisson_residual_synth_workspace_bytes(_lib.i64(cshape)) > 0
    assert per_member % (8 * 4 * 8) == 0 and per_member // (8 * 4 * 8) > 1
    nsums, npart = ops.residual_synth_batch_workspace(cshape)
    assert nsums == per_member // 8 and 1 <= npart <= 65536
    assert lib.odil_poisson_residual_synth_batch_workspace_bytes(_lib.i64((1, 4, 8))) == 0  # (a coarse extent below 2)
    assert lib.odil_poisson_residual_synth_batch_partials(_lib.i64((1, 4, 8))) == 0
    assert lib.odil_poisson_residual_synth_batch_workspace_bytes(None) == 0


def _refused(lib, entry, status, text):
    assert status == -1, (entry, text, status)
    err = lib.odil_last_error()
    assert entry.encode() in err and text in err, (entry, text, err)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_residual_launcher_refuses_before_launching(suffix):
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_poisson_residual_synth_batch_" + suffix)
    h2 = np.array([0.25, 0.5, 0.3], dtype=np.float64 if suffix == "f64" else np.float32)
    cshape, cells = (8, 4, 8), 8 * 256
    npart = lib.odil_poisson_residual_synth_batch_partials(_lib.i64(cshape))
    sums = lib.odil_poisson_residual_synth_batch_workspace_bytes(_lib.i64(cshape))
    assert npart >= 1 and sums >= 8 * 4 * 8

    def launch(nbatch=3, sw=cells, sr=cells, sf=cells, shp=cshape, ndim=3, pstride=npart, plen=None, sums_size=None,
               null=None, base=4096):
        ptrs = [c_void_p(base * (k + 1)) for k in range(7)]  # coarse w0 rhs fu partials column_sums loss
        flat, h2p = _lib.i64(shp), h2.ctypes.data_as(c_void_p)
        if null is not None:
            if null == 7:
                flat = None
            elif null == 8:
                h2p = None
            else:
                ptrs[null] = None
        plen = (nbatch - 1) * pstride + npart if plen is None else plen
        sums_size = max(nbatch, 0) * sums if sums_size is None else sums_size
        return fn(ptrs[0], ptrs[1], ptrs[2], ptrs[3], c_int(nbatch), c_int64(sw), c_int64(sr), c_int64(sf), flat, c_int(ndim),
                  h2p, ptrs[4], c_int64(pstride), c_int64(plen), ptrs[5], c_size_t(sums_size), ptrs[6], None)

    refused = lambda text, **kw: _refused(lib, "poisson_residual_synth_batch", launch(**kw), text)
    for k in range(9):
        refused(b"null pointer", null=k)
    for nbatch in (0, -1, 65536):
        refused(b"members", nbatch=nbatch)
    for key in ("sw", "sr", "sf"):
        refused(b"smaller than a member", **{key: cells - 1})
        refused(b"smaller than a member", **{key: 0})
        refused(b"not a multiple of 16 bytes", **{key: cells + 1})
    refused(b"too small", pstride=npart - 1)
    refused(b"too small", plen=2 * npart + npart - 1)  # (three members: two rows and all but one double of the third)
    refused(b"too small", plen=0)
    refused(b"column sums need", sums_size=3 * sums - 8)
    refused(b"column sums need", sums_size=0)
    refused(b"ndim 2", ndim=2)
    refused(b"ndim 4", ndim=4)
    # a grid beyond one launch, a coarse extent below 2, arrays off the grid of the 16-byte pairs
    status = launch(shp=(1 << 28, 1 << 28, 8), sw=1 << 62, sr=1 << 62, sf=1 << 62)
    assert status == -1 and b"grid too large for one launch" in lib.odil_last_error()
    assert launch(shp=(8, 1, 8)) == -1 and b"coarse extent 1" in lib.odil_last_error()
    assert launch(base=4100) == -1 and b"aligned" in lib.odil_last_error()


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_adjoint_launcher_refuses_before_launching(suffix):
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_poisson_adjoint_adam_volumes_" + suffix)
    h2 = np.array([0.25, 0.5, 0.3], dtype=np.float64 if suffix == "f64" else np.float32)
    shape, cells = (8, 4, 8), 256

    def launch(nbatch=3, strides=(cells,) * 5, shp=shape, ndim=3, astride=1, null=None):
        ptrs = [c_void_p(4096 * (k + 1)) for k in range(6)]  # fu g x m v alpha_dev
        flat, h2p = _lib.i64(shp), h2.ctypes.data_as(c_void_p)
        if null is not None:
            if null == 6:
                flat = None
            elif null == 7:
                h2p = None
            else:
                ptrs[null] = None
        return fn(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], c_int(nbatch), *[c_int64(s) for s in strides], flat,
                  c_int(ndim), h2p, 0.01, 0.1, 0.001, 1e-7, ptrs[5], c_int64(astride), None)

    refused = lambda text, **kw: _refused(lib, "poisson_adjoint_adam_volumes", launch(**kw), text)
    for k in (0, 2, 3, 4, 5, 6, 7):  # (g may be null: the gradient is then not stored)
        refused(b"null pointer", null=k)
    for nbatch in (0, -1, 65536):
        refused(b"members", nbatch=nbatch)
    for k in range(5):
        for bad, text in ((cells - 1, b"smaller than a member"), (cells + 1, b"not a multiple of 16 bytes")):
            strides = [cells] * 5
            strides[k] = bad
            refused(text, strides=tuple(strides))
    refused(b"negative", astride=-1)
    refused(b"ndim 2", ndim=2, shp=(16, 8))
    refused(b"ndim 1", ndim=1, shp=(16,))
    big = (1 << 20, 1 << 20, 8)  # a grid beyond one launch
    assert launch(shp=big, strides=(1 << 62,) * 5) == -1 and b"grid too large for one launch" in lib.odil_last_error()
    # the 1-D / 2-D entry point keeps refusing volumes
    old = getattr(lib, "odil_poisson_adjoint_adam_batch_" + suffix)
    ptrs = [c_void_p(4096 * (k + 1)) for k in range(6)]
    status = old(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], c_int(3), *[c_int64(cells)] * 5, _lib.i64(shape), c_int(3),
                 h2.ctypes.data_as(c_void_p), 0.01, 0.1, 0.001, 1e-7, ptrs[5], c_int64(1), None)
    _refused(lib, "poisson_adjoint_adam_batch", status, b"ndim 3")


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_transfer_launcher_refuses_before_launching(suffix):
    """The one transposed chain (odil_mg_synth_adj_adam_members) as the 3-D ensembles call it: loc 'ccc', the members as
    its rows."""
    from odil_amd import _lib, fused

    lib = _lib.load()
    fn = getattr(lib, "odil_mg_synth_adj_adam_members_" + suffix)
    shapes = [(16, 8, 8), (8, 4, 4), (4, 2, 2)]

    def launch(nbatch=3, shp=shapes, ndim=3, loc=None, astride=1, null=None, null_level=None, gu=1 << 20, odd_level=False):
        nlvl = len(shp)
        tables = []
        for k in range(4):  # grads x m v: HOST arrays of (dummy) device pointers
            arr = (c_void_p * nlvl)(*[4096 * (16 * k + l + 1) for l in range(nlvl)])
            if null_level == k:
                arr[1] = None
            if odd_level and k == 0:
                arr[1] = 4096 * 2 + 8
            tables.append(arr)
        ptrs = [c_void_p(gu), tables[0], _lib.i64([n for s in shp for n in s]), tables[1], tables[2], tables[3],
                c_void_p(1 << 21)]  # gu grads shapes x m v alpha_dev
        if null is not None:
            ptrs[null] = None
        loc = ("c" * ndim).encode() if loc is None else loc
        return fn(ptrs[0], ptrs[1], ptrs[2], c_int(nlvl), c_int(ndim), loc, c_int(nbatch), ptrs[3], ptrs[4], ptrs[5], 0.1,
                  0.001, 1e-7, ptrs[6], c_int64(astride), c_int64(0), None)

    refused = lambda text, **kw: _refused(lib, "mg_synth_adj_adam_members", launch(**kw), text)
    for k in range(7):
        refused(b"null pointer", null=k)
    for k in range(4):
        refused(b"null level array", null_level=k)
    for nbatch in (0, -1, 65536):
        refused(b"rows (1 ... 65535)", nbatch=nbatch)  # (the members are the chain's rows)
    refused(b"negative", astride=-1)
    refused(b"nlvl=1", shp=shapes[:1])
    # the chain itself takes 1-D to 4-D rows: that the volumes form runs 3-D members only is `volumes_refusal`'s rule
    assert "2-D grid: the batched launches of volumes run 3-D grids" in fused.volumes_refusal([(8, 8), (4, 4)])
    refused(b"loc of another length", ndim=2, shp=[(8, 8), (4, 4)], loc=b"ccc")
    refused(b"ndim 5", ndim=5, shp=[(8,) * 5, (4,) * 5])
    refused(b"not aligned to 16 bytes", gu=(1 << 20) + 8)
    refused(b"not aligned to 16 bytes", odd_level=True)
    assert launch(shp=[(16, 8, 8), (8, 4, 3)]) == -1 and b"does not refine" in lib.odil_last_error()
    assert launch(shp=[(4, 2, 2), (2, 1, 1)]) == -1 and b"must be >= 2" in lib.odil_last_error()
    # 65535 members of a level that one member runs through the fast kernel (coarse z extent below 4) cannot be counted
    # in its schedule: refused, not rerouted
    wide = [(4, 1 << 14, 1 << 14), (2, 1 << 13, 1 << 13)]
    refused(b"would not run the transposed prolongation one row runs", nbatch=65535, shp=wide)


def test_levels_query_and_kernel_kinds():
    """odil_mg_members_levels_ok on 'ccc' rows / odil_interp_adj_kind, from shapes alone: the levels of the shapes the GPU tests run take
    the same kernel for one member and for a batch, and the kinds are the ones the GPU tests mean to reach."""
    from odil_amd import _lib, fused

    lib = _lib.load()
    kind = lambda shape, loc, item: lib.odil_interp_adj_kind(_lib.i64(shape), len(shape), loc.encode(), item)
    FAST, ROWS, TILE, MARCH = 1, 3, 4, 5
    assert kind((2, 2, 2), "ccc", 8) == kind((70, 2, 2, 2), ".ccc", 8) == FAST  # tiny levels: coarse z extent below 4
    assert kind((16, 16, 16), "ccc", 8) == kind((70, 16, 16, 16), ".ccc", 8) == MARCH
    assert kind((4, 16, 64), "ccc", 8) == kind((70, 4, 16, 64), ".ccc", 8) == TILE
    assert kind((4, 16, 64), "ccc", 4) == kind((70, 4, 16, 64), ".ccc", 4) == ROWS  # float rows of 128 fine cells
    assert kind((4, 4, 32), "ccc", 4) == kind((3, 4, 4, 32), ".ccc", 4) == ROWS and kind((4, 4, 32), "ccc", 8) == MARCH
    assert kind((4, 16, 256), "ccc", 4) == kind((3, 4, 16, 256), ".ccc", 4) == TILE
    assert kind((4, 4), "cc", 8) == FAST and kind((4, 4, 4), "ccc", 2) < 0 and lib.odil_interp_adj_kind(None, 3, b"ccc", 8) < 0
    ok = lambda shapes, nb, item=8, loc=b"ccc": lib.odil_mg_members_levels_ok(_lib.i64([n for s in shapes for n in s]),
                                                                              len(shapes), len(shapes[0]), loc, nb, item)
    halves = lambda shape, nlvl: [tuple(n >> l for n in shape) for l in range(nlvl)]
    for shapes in (halves((4, 4, 4), 2), halves((8, 12, 20), 3), halves((8, 40, 80), 2), halves((64, 8, 16), 3),
                   halves((8, 32, 128), 3), halves((32, 32, 32), 4), halves((64, 64, 64), 5)):
        for nb in (1, 3, 70, 65535):
            for item in (8, 4):
                assert ok(shapes, nb, item) == 0, (shapes, nb, item, lib.odil_last_error())
    assert ok([(8, 8), (4, 4)], 3) == -1 and b"loc of another length" in lib.odil_last_error()  # (loc b"ccc", two axes)
    assert ok([(8, 8, 8)], 3) == -1 and b"nlvl=1" in lib.odil_last_error()
    assert ok(halves((8, 8, 8), 2), 0) == -1 and b"rows (1 ... 65535)" in lib.odil_last_error()
    assert ok(halves((8, 8, 8), 2), 3, 2) == -1 and b"element size" in lib.odil_last_error()
    wide = [(4, 1 << 14, 1 << 14), (2, 1 << 13, 1 << 13)]
    assert fused._levels_refusal(wide, 1, torch.float64) is None
    assert "would not run the transposed prolongation one row runs" in fused._levels_refusal(wide, 65535, torch.float64)
    # the query answers for 1-D to 4-D rows: that a form runs members of its dimensions only is the form's own rule
    assert ok([(8, 8), (4, 4)], 3, loc=b"cc") == 0 and "2-D grid" in fused.volumes_refusal([(8, 8), (4, 4)], torch.float64)
    assert ok(halves((8, 8, 8), 2), 3) == 0 and "3-D grid" in fused.launches_refusal(halves((8, 8, 8), 2))


def test_the_form_is_a_function_of_shapes_and_dtype():
    from odil_amd import fused

    f64, f32 = torch.float64, torch.float32
    halves = lambda shape, nlvl: [tuple(n >> l for n in shape) for l in range(nlvl)]
    for dtype in (f64, f32):
        assert fused.ensemble_form("auto", halves((16, 16, 16), 3), dtype) == "volumes"
        assert fused.ensemble_form("auto", halves((8, 12, 20), 3), dtype) == "volumes"
        assert fused.ensemble_form("auto", [(8, 8, 8)], dtype) == "volumes"  # (then refused by volumes_refusal: one level)
    # the 1-D / 2-D answers are the ones they were
    assert fused.ensemble_form("auto", halves((256,), 8), f64) == "workgroup"
    assert fused.ensemble_form("auto", halves((256,), 8), f32) == "workgroup"
    assert fused.ensemble_form("auto", [(128, 128), (64, 64)], f64) == "launches"
    assert fused.ensemble_form("auto", [(40, 94), (20, 47)], f64) == "launches"
    assert fused.ensemble_form("auto", [(40, 94), (20, 47)], f32) == "workgroup"
    assert fused.ensemble_form("auto", halves((8192,), 5), f64) == "launches"
    for form in ("workgroup", "launches", "volumes"):
        assert fused.ensemble_form(form, [(128, 128), (64, 64)], f64) == form
        assert fused.ensemble_form(form, halves((16, 16, 16), 2), f64) == form
    with pytest.raises(ValueError, match="form 'bogus'"):
        fused.ensemble_form("bogus", [(16, 16, 16), (8, 8, 8)], f64)
    # the other forms keep their 3-D reasons
    assert "a 3-D run fuses the synthesis into its residual and the first transpose into its adjoint" in fused.launches_refusal(
        halves((8, 8, 8), 2))
    assert "3-D grid: the one-workgroup epochs run 1-D and 2-D grids" in fused.small_refusal(halves((8, 8, 8), 2), f64)


def test_volumes_refusal_gives_each_of_its_reasons():
    from odil_amd import fused

    f64, f32 = torch.float64, torch.float32
    halves = lambda shape, nlvl: [tuple(n >> l for n in shape) for l in range(nlvl)]
    for shapes in (halves((4, 4, 4), 2), halves((8, 12, 20), 3), halves((8, 40, 80), 2), halves((64, 8, 16), 3),
                   halves((32, 32, 32), 4), halves((64, 64, 64), 5), halves((16, 16, 16), 3)):
        assert fused.volumes_refusal(shapes, f64) is None and fused.volumes_refusal(shapes, f32) is None, shapes
        assert fused.volumes_refusal(shapes) is None
    assert "2-D grid" in fused.volumes_refusal([(64, 64), (32, 32)], f64)
    assert "1-D grid" in fused.volumes_refusal([(64,), (32,)], f64)
    assert "at least 2 levels" in fused.volumes_refusal([(16, 16, 16)], f64)
    assert "halve" in fused.volumes_refusal([(12, 12, 12), (6, 6, 6), (3, 3, 2)], f64)
    assert "halve" in fused.volumes_refusal([(9, 8, 8), (4, 4, 4)], f64)
    assert "finest level must be at least 4" in fused.volumes_refusal([(2, 4, 4), (1, 2, 2)], f64)
    assert "finest level must be at least 4" in fused.volumes_refusal([(2, 2, 2), (1, 1, 1)], f64)
    # members lie back to back: every member must start on a 16-byte boundary
    assert "16 bytes" in fused.volumes_refusal([(3, 3, 3), (2, 2, 2)], f32)
    assert "16 bytes" in fused.volumes_refusal([(3, 3, 3), (2, 2, 2)], f64)
    # the limits of the kernels are the library's
    assert "nlvl=33" in fused.volumes_refusal([(1 << (34 - l),) * 3 for l in range(33)], f64)
    # a member whose single run takes the one-pass adjoint + transpose launch is admitted in float64; in float32 only
    # where the separate first transpose is not the row-marching kernel, whose sums round differently
    assert fused.volumes_refusal(halves((8, 32, 128), 3), f64) is None
    assert fused.volumes_refusal(halves((8, 32, 512), 2), f32) is None
    assert "one-pass" in fused.volumes_refusal(halves((8, 32, 128), 3), f32)
    assert "one-pass" in fused.volumes_refusal(halves((16, 64, 256), 2), f32)
    assert fused.volumes_refusal(halves((8, 16, 128), 2), f32) is None  # (no one-pass launch below 32 rows)


# ------------------------------------------------------------------------------------------- optimize_ensemble
@pytest.fixture()
def api(monkeypatch):
    """(odil, the Poisson example) with the process-wide `mod` on CPU tensors: problems and states can be built, nothing
    can be computed."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    return odil, poisson


def stretched(odil, poisson):
    """The 3-D N = 16 problem on a box twice as long: same shapes, another spacing."""
    import argparse

    domain = odil.Domain(cshape=[16, 16, 16], multigrid=True, dtype=np.float64, upper=2.0)
    state = domain.init_state(odil.State(fields={"u": None}))
    extra = argparse.Namespace(rhs=domain.points()[0] * 0, args=argparse.Namespace(mgloss=0))
    return odil.Problem(poisson.operator, domain, extra), state


def members(odil, poisson, specs):
    out = [stretched(odil, poisson) if spec == "stretched" else poisson.make_problem(poisson.parse_args(spec.split()))
           for spec in specs]
    args = poisson.parse_args(specs[0].split())
    args.epoch_start, args.epochs = 0, 5
    return args, [p for p, _ in out], [s for _, s in out]


@pytest.mark.parametrize("form", ["volumes", "auto"])
@pytest.mark.parametrize("specs,member,reason", [
    (["--ndim 3 --N 16", "--ndim 2 --N 64", "--ndim 3 --N 16"], 1, "2-D grid: the batched launches of volumes run 3-D grids"),
    (["--ndim 3 --N 16", "--ndim 3 --N 16", "--ndim 3 --N 16 --multigrid 0"], 2, "at least 2 levels"),
    (["--ndim 3 --N 16 --multigrid 0"], 0, "at least 2 levels"),
    (["--ndim 3 --N 16", "--ndim 3 --N 32"], 1, "level shapes .* differ from member 0"),
    (["--ndim 3 --N 16 --double 0", "--ndim 3 --N 16"], 1, "dtype"),
    (["--ndim 3 --N 16", "--ndim 3 --N 16", "stretched"], 2, "grid spacing"),
], ids=["2d-member", "one-level-member", "one-level-alone", "mixed-size", "mixed-dtype", "mixed-spacing"])
def test_volumes_form_names_the_first_offending_member(api, specs, member, reason, form):
    """From the shapes alone, before any operator is probed (so before any device is needed)."""
    odil, poisson = api
    args, problems, states = members(odil, poisson, specs)
    with pytest.raises(ValueError, match="member {}: .*{}".format(member, reason)):
        odil.util.optimize_ensemble(args, problems, states, form=form)


def test_the_other_forms_keep_refusing_volumes(api):
    odil, poisson = api
    args, problems, states = members(odil, poisson, ["--ndim 3 --N 16"] * 2)
    with pytest.raises(ValueError, match="member 0: 3-D grid: the batched launches run 1-D and 2-D grids "
                                         r"\(a 3-D run fuses the synthesis into its residual and the first transpose into its adjoint\)"):
        odil.util.optimize_ensemble(args, problems, states, form="launches")
    with pytest.raises(ValueError, match="member 0: 3-D grid: the one-workgroup epochs run 1-D and 2-D grids"):
        odil.util.optimize_ensemble(args, problems, states)
    with pytest.raises(ValueError, match="form 'bogus'"):
        odil.util.optimize_ensemble(args, problems, states, form="bogus")
    for problem, state in zip(problems, states):  # (all the volumes form asks before it probes the operators)
        from odil_amd import fused

        arrays = problem.domain.arrays_from_state(state)
        shapes = [tuple(int(n) for n in a.shape) for a in arrays]
        assert len(shapes) >= 2 and fused.volumes_refusal(shapes, arrays[0].dtype) is None
