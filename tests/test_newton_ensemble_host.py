"""Newton steps for ensembles of Poisson problems (odil_stencil_solve_batch, gmg.EnsembleGMG, util.optimize_newton_ensemble)
as far as they can be checked without a device: header, library and binding agree on the entry points, the launcher
refuses malformed arguments with an error text before anything is launched (the pointers are dummies), `fused.newton_refusal`
gives each of its reasons, and `optimize_newton_ensemble` names the first member that cannot join -- from shapes alone."""

import argparse
import os
import sys
from ctypes import c_double, c_float, c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("odil_stencil_solve_batch_f64", "odil_stencil_solve_batch_f32", "odil_stencil_solve_batch_work")


def test_header_library_and_binding_agree():
    from odil_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTED and name + "(" in header, name
    assert all(getattr(lib, name).argtypes for name in NAMES)


def test_work_elements_per_member():
    """Three arrays per level (iterate, spare, right-hand side; the finest level's third holds the Newton residual, so mode
    1 adds nothing); 0 for malformed shapes."""
    from odil_amd import _lib

    work = _lib.load().odil_stencil_solve_batch_work
    assert work(_lib.i64([64, 32, 16]), 3, 1) == 3 * (64 + 32 + 16)
    assert work(_lib.i64([12, 20, 6, 10, 3, 5]), 3, 2) == 3 * (240 + 60 + 15)
    assert work(_lib.i64([8, 4, 16, 4, 2, 8]), 2, 3) == 3 * (512 + 64)
    assert work(_lib.i64([32768]), 1, 1) == 3 * 32768
    assert work(None, 1, 1) == 0
    assert work(_lib.i64([64]), 0, 1) == 0 and work(_lib.i64([2] * 9), 9, 1) == 0
    assert work(_lib.i64([64]), 1, 0) == 0 and work(_lib.i64([4] * 4), 1, 4) == 0
    assert work(_lib.i64([64, 0]), 2, 1) == 0 and work(_lib.i64([-4]), 1, 1) == 0
    assert work(_lib.i64([32769]), 1, 1) == 0
    assert work(_lib.i64([2048, 2048]), 1, 2) == 0  # (more than 2^20 cells)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_launcher_refuses_before_launching(suffix):
    """Every refusal of the launcher: ODIL_E_INVAL and a text that names the entry point and the reason.  The device pointers
    are dummies, so a launch that did happen could not succeed; none is attempted."""
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_stencil_solve_batch_" + suffix)
    real = c_double if suffix == "f64" else c_float
    npdt = np.float64 if suffix == "f64" else np.float32
    weights = np.array([0.5, 0.75, 1.0, 1.0], dtype=npdt)
    wp = weights.ctypes.data_as(c_void_p)
    shapes = [(16, 8), (8, 4), (4, 2)]
    cells, total, ncoeff, ninv = 128, 168, 5 * 168, 8
    need = 3 * total

    def launch(shp=shapes, halve=((1, 1), (1, 1)), ndim=2, nbatch=3, cs=0, xs=cells + 3, bs=cells + 1, ws=need + 5, wl=None,
               ins=0, ninv=ninv, npre=2, npost=2, start=2, mode=0, maxc=10, tol=1e-10, hs=12, null=None, alias=False,
               nohalve=False):
        ptrs = dict(coeffs=4096, x=8192, b=12288, work=16384, inv=20480, history=24576, outcome=28672)
        ptrs = {k: c_void_p(v) for k, v in ptrs.items()}
        ptrs.update(wpre=wp, wpost=wp)
        flat = _lib.i64([n for s in shp for n in s])
        values = [h for tr in halve for h in tr]
        mask = (c_int * max(1, len(values)))(*values)
        import ctypes

        maskp = None if nohalve else ctypes.cast(mask, c_void_p)
        if null == "shapes":
            flat = None
        elif null is not None:
            ptrs[null] = None
        if alias:
            ptrs["b"] = ptrs["x"]
        wl = (nbatch - 1) * ws + need if wl is None else wl
        return fn(ptrs["coeffs"], c_int64(cs), flat, maskp, c_int(len(shp)), c_int(ndim), c_int(nbatch), ptrs["x"], c_int64(xs),
                  ptrs["b"], c_int64(bs), ptrs["work"], c_int64(ws), c_int64(wl), ptrs["inv"], c_int64(ins), c_int(ninv),
                  ptrs["wpre"], c_int(npre), ptrs["wpost"], c_int(npost), c_int(start), c_int(mode), c_int(maxc), real(tol),
                  ptrs["history"], c_int64(hs), ptrs["outcome"], None)

    def refused(text, **kw):
        assert launch(**kw) == -1, kw
        err = lib.odil_last_error()
        assert b"stencil_solve_batch" in err and text in err, (kw, err)

    # what odil_stencil_vcycle_tail refuses
    refused(b"bad arguments", shp=[(2,)] * 9, halve=[(0,)] * 8, ndim=1)
    refused(b"bad arguments", ndim=4)
    refused(b"bad arguments", ndim=0)
    refused(b"bad arguments", npre=5)
    refused(b"bad arguments", npost=-1)
    refused(b"extent", shp=[(16, 0), (8, 0)], halve=((1, 1),))
    refused(b"extent", shp=[(40000,)], halve=(), ndim=1)
    refused(b"does not follow", shp=[(16, 8), (8, 4), (4, 3)])
    refused(b"does not follow", shp=[(16, 8), (7, 4)], halve=((1, 1),))
    refused(b"does not follow", shp=[(16, 8), (8, 8)], halve=((1, 1),))
    refused(b"does not follow", shp=[(15, 8), (7, 4)], halve=((1, 1),))
    refused(b"cells", shp=[(2048, 1024)], halve=())
    refused(b"the inverse", ninv=7)
    # a null pointer
    for name in ("coeffs", "shapes", "x", "b", "work", "inv", "history", "outcome", "wpre", "wpost"):
        refused(b"null pointer", null=name)
    refused(b"null pointer", nohalve=True)
    # the members
    for nbatch in (0, -1, 65536):
        refused(b"members", nbatch=nbatch)
    # strides below a member's need, a work array that does not hold every member
    refused(b"smaller than a member", xs=cells - 1)
    refused(b"smaller than a member", bs=cells - 1)
    refused(b"smaller than a member", ws=need - 1)
    refused(b"smaller than a member", xs=0)
    refused(b"work array", wl=2 * (need + 5) + need - 1)
    refused(b"work array", wl=0)
    # shared (0) or per member
    refused(b"neither 0", cs=ncoeff - 1)
    refused(b"neither 0", ins=ninv * ninv - 1)
    refused(b"neither 0", cs=1)
    for name in ("cs", "xs", "bs", "ws", "ins", "hs"):
        refused(b"negative stride", **{name: -1})
    refused(b"history_stride", hs=11)
    refused(b"history_stride", hs=0)
    refused(b"maxcycles", maxc=-1)
    refused(b"maxcycles", maxc=1001, hs=2000)
    refused(b"start", start=3)
    refused(b"start", start=-1)
    refused(b"mode", mode=2)
    refused(b"mode", mode=-1)
    refused(b"Newton step starts from", mode=1, start=1)
    refused(b"negative tol", tol=-1e-3)
    refused(b"alias", alias=True)


# ----------------------------------------------------------------------------------------------- fused.newton_refusal
def h2_of(shape, upper=1.0):
    return [(upper / n) ** 2 for n in shape]


def test_newton_refusal_gives_each_reason():
    from odil_amd import fused

    f64 = torch.float64
    assert "4-D" in fused.newton_refusal((8,) * 4, h2_of((8,) * 4), f64)
    assert "262144 cells are above the limit" in fused.newton_refusal((64,) * 3, h2_of((64,) * 3), f64)
    assert "65536 cells are above the limit" in fused.newton_refusal((256, 256), h2_of((256, 256)), f64)
    assert "65536 cells are above the limit" in fused.newton_refusal((65536,), h2_of((65536,)), f64)
    assert "cells too far from cubes" in fused.newton_refusal((1024, 64), h2_of((1024, 64)), f64)
    assert "cells too far from cubes" in fused.newton_refusal((64, 16), h2_of((64, 16)), torch.float32)
    reason = fused.newton_refusal((100, 100), h2_of((100, 100)), f64)
    assert "coarsest level (25, 25) has 625 unknowns" in reason


@pytest.mark.parametrize("shape", [(64,), (32768,), (12, 20), (128, 128), (16,) * 3, (32,) * 3])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_newton_refusal_admits(shape, dtype):
    from odil_amd import fused, gmg

    h2 = [(1.0 / 16) ** 2] * len(shape) if shape == (12, 20) else h2_of(shape)  # (equal spacing on every axis)
    assert fused.newton_refusal(shape, h2, dtype) is None
    shapes, h2s, locs, min_size = gmg.EnsembleGMG.plan(shape, h2, np.float64)
    assert len(shapes) <= 8 and int(np.prod(shapes[-1])) <= 512 and all(loc == "c" * len(shape) for loc in locs)
    if shape == (32768,):  # PoissonGMG would build 15 levels: cut where 8 remain
        assert shapes[-1] == (256,) and len(shapes) == 8 and min_size == 256
        assert gmg.poisson_hierarchy(shape, h2, np.float64, min_size)[0] == shapes


# ------------------------------------------------------------------------------------------ optimize_newton_ensemble
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
    """The 1-D N = 64 problem with a plain unknown on a box twice as long: same shape, another spacing."""
    domain = odil.Domain(cshape=[64], multigrid=False, dtype=np.float64, upper=2.0)
    state = domain.init_state(odil.State(fields={"u": None}))
    extra = argparse.Namespace(rhs=domain.points()[0] * 0, args=argparse.Namespace(mgloss=0))
    return odil.Problem(poisson.operator, domain, extra), state


BASE = "--multigrid 0 --optimizer newton --linsolver multigrid "


def members(odil, poisson, specs):
    out = [stretched(odil, poisson) if spec == "stretched" else poisson.make_problem(poisson.parse_args((BASE + spec).split()))
           for spec in specs]
    args = poisson.parse_args((BASE + specs[0]).split())
    args.epoch_start, args.epochs = 0, 2
    return args, [p for p, _ in out], [s for _, s in out]


@pytest.mark.parametrize("specs,member,reason", [
    (["--ndim 1 --N 64", "--ndim 1 --N 64", "--ndim 1 --N 128"], 2, "cells .* differ from member 0"),
    (["--ndim 2 --N 16", "--ndim 1 --N 16"], 1, "cells .* differ from member 0"),
    (["--ndim 1 --N 64 --double 0", "--ndim 1 --N 64"], 1, "dtype"),
    (["--ndim 1 --N 64", "--ndim 1 --N 64", "stretched"], 2, "grid spacing"),
    (["--ndim 1 --N 64", "--ndim 1 --N 64 --multigrid 1"], 1, "MultigridField .*no multigrid decomposition"),
    (["--ndim 2 --N 16", "--ndim 3 --N 64"], 1, "262144 cells are above the limit"),
    (["--ndim 2 --N 100"], 0, "coarsest level .* 625 unknowns"),
], ids=["mixed-size", "mixed-ndim", "mixed-dtype", "mixed-spacing", "multigrid-member", "above-limit", "coarsest"])
def test_names_the_first_offending_member(api, specs, member, reason):
    """Members that cannot run side by side raise ValueError with their index and the reason -- from the shapes alone,
    before any operator is probed (so before any device is needed)."""
    odil, poisson = api
    args, problems, states = members(odil, poisson, specs)
    with pytest.raises(ValueError, match="optimize_newton_ensemble: member {}: .*{}".format(member, reason)):
        odil.util.optimize_newton_ensemble(args, problems, states)


def test_refuses_other_solvers_damping_and_count_mismatch(api):
    odil, poisson = api
    args, problems, states = members(odil, poisson, ["--ndim 1 --N 64"] * 2)
    with pytest.raises(ValueError, match="optimize_newton_ensemble: 2 problems with 1 states"):
        odil.util.optimize_newton_ensemble(args, problems, states[:1])
    with pytest.raises(ValueError, match="optimize_newton_ensemble: 0 problems"):
        odil.util.optimize_newton_ensemble(args, [], [])
    for linsolver in ("cg", "bicgstab", "lsqr", "directsq"):
        args.linsolver = linsolver
        with pytest.raises(ValueError, match="optimize_newton_ensemble: linsolver '{}'".format(linsolver)):
            odil.util.optimize_newton_ensemble(args, problems, states)
    args.linsolver = "multigrid"
    for name in ("linsolver_damp", "linsolver_dampdiag"):
        setattr(args, name, 0.1)
        with pytest.raises(ValueError, match="optimize_newton_ensemble: damping"):
            odil.util.optimize_newton_ensemble(args, problems, states)
        setattr(args, name, 0)


def test_optimize_ensemble_still_refuses_newton(api):
    odil, poisson = api
    args, problems, states = members(odil, poisson, ["--ndim 1 --N 64"] * 2)
    args.optimizer = "newton"
    with pytest.raises(ValueError, match="Adam.*'newton'"):
        odil.util.optimize_ensemble(args, problems, states)
