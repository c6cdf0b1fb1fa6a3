"""The ensemble of Poisson problems as batched launches (odil_poisson_residual_batch, odil_poisson_adjoint_adam_batch,
odil_mg_synth_adj_adam_members, fused.PoissonLaunchEnsemble, util.optimize_ensemble(form=...)) as far as it can be checked
without a device: the library exports the entry points and header, library and `_lib.EXPORTED` agree; the launchers refuse
malformed arguments with an error text before anything is launched (every pointer is a dummy, so a launch that did happen
could not succeed: tests/test_ensemble_host.py is the model); `optimize_ensemble` names the first member that cannot join,
from shapes alone; and the choice between the two forms is a function of shapes and dtype."""

import os
import re
import sys
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["odil_poisson_residual_batch", "odil_poisson_adjoint_adam_batch", "odil_mg_synth_adj_adam_members"]


def test_library_header_and_bindings_agree_on_the_new_entry_points():
    from odil_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    declared = set(re.findall(r"\b(odil_\w+)\s*\(", header))
    names = [n + s for n in NEW for s in ("_f64", "_f32")] + ["odil_poisson_batch_partials"]
    for name in names:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
        assert name in declared, name
    # every exported name is declared and present (the whole table, so that the three cannot drift apart)
    for name in _lib.EXPORTED:
        assert hasattr(lib, name) and name in declared, name
    # a member's row of the partials workspace: one double per workgroup of the residual kernel's schedule
    part = lib.odil_poisson_batch_partials
    assert part(_lib.i64([64, 64]), 2, 8) == 64 * 1  # 64 rows, one x segment of 256 lanes x 2
    assert 12 * 3 <= part(_lib.i64([12, 1040]), 2, 8) < 12 * 3 + 8  # 1040 / 512 -> 3 x segments (+ padding to 8 XCDs)
    assert 12 * 2 <= part(_lib.i64([12, 1040]), 2, 4) < 12 * 2 + 8  # 1040 / 1024 -> 2
    assert part(_lib.i64([8192]), 1, 8) == 16
    assert part(_lib.i64([8, 8, 8]), 3, 8) == 0 and part(None, 1, 8) == 0 and part(_lib.i64([8]), 1, 2) == 0


def _refused(lib, entry, status, text):
    assert status == -1, (entry, text, status)
    err = lib.odil_last_error()
    assert entry.encode() in err and text in err, (entry, text, err)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_residual_launcher_refuses_before_launching(suffix):
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_poisson_residual_batch_" + suffix)
    item = 8 if suffix == "f64" else 4
    h2 = np.array([0.25, 0.5], dtype=np.float64 if suffix == "f64" else np.float32)
    shape, cells = (16, 8), 128
    npart = lib.odil_poisson_batch_partials(_lib.i64(shape), 2, item)
    assert npart >= 1

    def launch(nbatch=3, su=cells, sr=cells, sf=cells, shp=shape, ndim=2, pstride=npart, plen=None, null=None):
        ptrs = [c_void_p(4096 * (k + 1)) for k in range(5)]  # u rhs fu partials loss
        flat, h2p = _lib.i64(shp), h2.ctypes.data_as(c_void_p)
        if null is not None:
            if null == 5:
                flat = None
            elif null == 6:
                h2p = None
            else:
                ptrs[null] = None
        plen = (nbatch - 1) * pstride + npart if plen is None else plen
        return fn(ptrs[0], ptrs[1], ptrs[2], c_int(nbatch), c_int64(su), c_int64(sr), c_int64(sf), flat, c_int(ndim), h2p,
                  ptrs[3], c_int64(pstride), c_int64(plen), ptrs[4], None)

    refused = lambda text, **kw: _refused(lib, "poisson_residual_batch", launch(**kw), text)
    for k in range(7):
        refused(b"null pointer", null=k)
    for nbatch in (0, -1, 65536):
        refused(b"members", nbatch=nbatch)
    for key in ("su", "sr", "sf"):
        refused(b"smaller than a member", **{key: cells - 1})
        refused(b"smaller than a member", **{key: 0})
        refused(b"not a multiple of 16 bytes", **{key: cells + 1})
    refused(b"not a multiple of 16 bytes", shp=(16, 9), su=16 * 9 + 1, sr=16 * 9 + 1, sf=16 * 9 + 1)  # (rows no whole packs)
    refused(b"too small", pstride=npart - 1)
    refused(b"too small", plen=2 * npart + npart - 1)  # (three members: two rows and all but one double of the third)
    refused(b"too small", plen=0)
    refused(b"ndim 3", ndim=3, shp=(4, 4, 4))
    refused(b"ndim 0", ndim=0)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_adjoint_launcher_refuses_before_launching(suffix):
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_poisson_adjoint_adam_batch_" + suffix)
    h2 = np.array([0.25, 0.5], dtype=np.float64 if suffix == "f64" else np.float32)
    shape, cells = (16, 8), 128

    def launch(nbatch=3, strides=(cells,) * 5, shp=shape, ndim=2, astride=1, null=None):
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

    refused = lambda text, **kw: _refused(lib, "poisson_adjoint_adam_batch", launch(**kw), text)
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
    refused(b"ndim 3", ndim=3, shp=(4, 4, 4))


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_transfer_launcher_refuses_before_launching(suffix):
    """The one transposed chain (odil_mg_synth_adj_adam_members) as the 1-D / 2-D ensembles call it: loc 'c' / 'cc', the
    members as its rows."""
    from odil_amd import _lib, fused

    lib = _lib.load()
    fn = getattr(lib, "odil_mg_synth_adj_adam_members_" + suffix)
    shapes = [(16, 8), (8, 4), (4, 2)]

    def launch(nbatch=3, shp=shapes, ndim=2, loc=None, astride=1, period=0, null=None, null_level=None, gu=1 << 20,
               odd_level=False):
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
                  0.001, 1e-7, ptrs[6], c_int64(astride), c_int64(period), None)

    refused = lambda text, **kw: _refused(lib, "mg_synth_adj_adam_members", launch(**kw), text)
    for k in range(7):
        refused(b"null pointer", null=k)
    for k in range(4):
        refused(b"null level array", null_level=k)
    for nbatch in (0, -1, 65536):
        refused(b"rows (1 ... 65535)", nbatch=nbatch)  # (the members are the chain's rows)
    refused(b"negative", astride=-1)
    refused(b"negative", period=-1)
    refused(b"nlvl=1", shp=shapes[:1])
    # the chain itself takes 1-D to 4-D rows: that the 1-D / 2-D form runs no volumes is `launches_refusal`'s rule
    assert "3-D grid: the batched launches run 1-D and 2-D grids" in fused.launches_refusal([(8, 8, 8), (4, 4, 4)])
    refused(b"ndim 5", ndim=5, shp=[(8,) * 5, (4,) * 5])
    refused(b"ndim 0", ndim=0)
    refused(b"loc of another length", loc=b"c")
    refused(b"every axis of a row is 'c' or 'n'", loc=b".c")
    refused(b"not aligned to 16 bytes", gu=(1 << 20) + 8)
    refused(b"not aligned to 16 bytes", odd_level=True)
    # levels that do not refine each other, and a coarsest level too small for the transfer's taps
    assert launch(shp=[(16, 8), (8, 3)]) == -1 and b"does not refine" in lib.odil_last_error()
    assert launch(shp=[(4, 2), (2, 1)]) == -1 and b"must be >= 2" in lib.odil_last_error()
    # a batch whose rows cannot be counted in 31 bits would leave the fast kernel a single member runs: refused, not rerouted
    # (1-D: the members are the rows of the '.c' layout, 65535 of them x 2^16 segments of 256 coarse cells)
    refused(b"would not run the transposed prolongation one row runs", nbatch=65535, ndim=1, shp=[(1 << 25,), (1 << 24,)])


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
    """The 2-D N = 64 problem on a box twice as long: same shapes, another spacing."""
    import argparse

    domain = odil.Domain(cshape=[64, 64], multigrid=True, dtype=np.float64, upper=2.0)
    state = domain.init_state(odil.State(fields={"u": None}))
    extra = argparse.Namespace(rhs=domain.points()[0] * 0, args=argparse.Namespace(mgloss=0))
    return odil.Problem(poisson.operator, domain, extra), state


def members(odil, poisson, specs):
    out = [stretched(odil, poisson) if spec == "stretched" else poisson.make_problem(poisson.parse_args(spec.split()))
           for spec in specs]
    args = poisson.parse_args(specs[0].split())
    args.epoch_start, args.epochs = 0, 5
    return args, [p for p, _ in out], [s for _, s in out]


def test_an_unknown_form_raises(api):
    odil, poisson = api
    args, problems, states = members(odil, poisson, ["--ndim 1 --N 64"] * 2)
    with pytest.raises(ValueError, match="form 'bogus'"):
        odil.util.optimize_ensemble(args, problems, states, form="bogus")


@pytest.mark.parametrize("specs,member,reason", [
    (["--ndim 2 --N 64", "--ndim 3 --N 16"], 1, "3-D grid: the batched launches run 1-D and 2-D"),
    (["--ndim 3 --N 8"], 0, "3-D grid: the batched launches run 1-D and 2-D"),
    (["--ndim 2 --N 64", "--ndim 2 --N 64", "--ndim 2 --N 64 --multigrid 0"], 2, "at least 2 levels"),
    (["--ndim 2 --N 64 --multigrid 0"], 0, "at least 2 levels"),
    (["--ndim 2 --N 64", "--ndim 2 --N 128"], 1, "level shapes .* differ from member 0"),
    (["--ndim 2 --N 64 --double 0", "--ndim 2 --N 64"], 1, "dtype"),
    (["--ndim 2 --N 64", "--ndim 2 --N 64", "stretched"], 2, "grid spacing"),
], ids=["3d-member", "3d-alone", "one-level-member", "one-level-alone", "mixed-size", "mixed-dtype", "mixed-spacing"])
def test_launches_form_names_the_first_offending_member(api, specs, member, reason):
    """From the shapes alone, before any operator is probed (so before any device is needed)."""
    odil, poisson = api
    args, problems, states = members(odil, poisson, specs)
    with pytest.raises(ValueError, match="member {}: .*{}".format(member, reason)):
        odil.util.optimize_ensemble(args, problems, states, form="launches")


@pytest.mark.parametrize("spec", ["--ndim 2 --N 128", "--ndim 1 --N 8192 --nlvl 5"])
def test_launches_form_does_not_refuse_on_size(api, spec):
    """What the workgroup form refuses on size ('cells are above the limit', 'N levels: ... at most 12') passes every structural check of the launches
    form: `launches_refusal` -- all that `optimize_ensemble(form="launches")` asks before it probes the operators, which
    needs a device -- admits the members' level shapes."""
    from odil_amd import fused

    odil, poisson = api
    args, problems, states = members(odil, poisson, [spec] * 2)
    with pytest.raises(ValueError, match="member 0: .*(above the limit|levels: the one-workgroup epochs take at most)"):
        odil.util.optimize_ensemble(args, problems, states)
    for problem, state in zip(problems, states):
        arrays = problem.domain.arrays_from_state(state)
        shapes = [tuple(int(n) for n in a.shape) for a in arrays]
        assert len(shapes) >= 2 and shapes[0] == tuple(problem.domain.cshape)
        assert fused.launches_refusal(shapes, arrays[0].dtype) is None
        assert fused.ensemble_form("auto", shapes, arrays[0].dtype) == "launches"


def test_the_form_is_a_function_of_shapes_and_dtype():
    from odil_amd import fused

    f64, f32 = torch.float64, torch.float32
    halves = lambda shape, nlvl: [tuple(n >> l for n in shape) for l in range(nlvl)]
    assert fused.ensemble_form("auto", halves((256,), 8), f64) == "workgroup"
    assert fused.ensemble_form("auto", halves((256,), 8), f32) == "workgroup"
    assert fused.ensemble_form("auto", [(128, 128), (64, 64)], f64) == "launches"
    assert fused.ensemble_form("auto", [(40, 94), (20, 47)], f64) == "launches"
    assert fused.ensemble_form("auto", [(40, 94), (20, 47)], f32) == "workgroup"  # (resident in float32)
    assert fused.ensemble_form("auto", halves((8192,), 5), f64) == "launches"
    for form in ("workgroup", "launches"):
        assert fused.ensemble_form(form, [(128, 128), (64, 64)], f64) == form
        assert fused.ensemble_form(form, halves((256,), 8), f64) == form
    with pytest.raises(ValueError, match="form"):
        fused.ensemble_form("bogus", [(16,), (8,)], f64)
    assert fused.launches_refusal([(128, 128), (64, 64)]) is None and fused.launches_refusal(halves((8192,), 5)) is None
    assert "3-D" in fused.launches_refusal([(8, 8, 8), (4, 4, 4)])
    assert "at least 2 levels" in fused.launches_refusal([(64, 64)])
    assert "halve" in fused.launches_refusal([(94,), (47,), (23,)])
    assert "at least 2" in fused.launches_refusal([(2, 4), (1, 2)])
    # members lie back to back: every member must start on a 16-byte boundary (1-D float32 with n = 2 mod 4 does not)
    assert "16 bytes" in fused.launches_refusal([(6,), (3,)], f32) and fused.launches_refusal([(6,), (3,)], f64) is None
    # the limits of the kernels are the library's: more levels than the transfer chains take, a batch beyond the schedule
    assert "nlvl=33" in fused.launches_refusal([(1 << (34 - l),) for l in range(33)])
    assert fused._levels_refusal([(1 << 25,), (1 << 24,)], 1) is None
    assert "would not run the transposed prolongation one row runs" in fused._levels_refusal([(1 << 25,), (1 << 24,)], 65535)
