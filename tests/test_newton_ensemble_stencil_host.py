"""Newton ensembles of variable-coefficient stencil problems as far as they can be checked without a device: the three
set-up entry points (odil_stencil_var_coarsen_batch, odil_stencil_strength_batch, odil_stencil_dense_batch) exist in header,
library and binding, their launchers refuse malformed arguments with an error text before anything is launched (the
pointers are dummies), `fused.newton_stencil_refusal` gives its reasons from the shape alone, and
`optimize_newton_ensemble` still names the first member that cannot join before it touches a state."""

import ctypes
import os
import sys
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["odil_stencil_{}_{}".format(stem, suffix) for stem in ("var_coarsen_batch", "strength_batch", "dense_batch")
         for suffix in ("f64", "f32")]


def test_header_library_and_binding_agree():
    from odil_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTED and name + "(" in header, name
        assert getattr(lib, name).argtypes and getattr(lib, name).restype is c_int


def test_ops_wrappers_exist():
    from odil_amd import ops

    assert all(callable(getattr(ops, name)) for name in ("stencil_var_coarsen_batch", "stencil_strength_batch",
                                                          "stencil_dense_batch"))


class Launchers:
    """The three entry points of one precision behind keyword arguments; the device pointers are dummies."""

    def __init__(self, suffix):
        from odil_amd import _lib

        self.lib = _lib.load()
        self.i64 = _lib.i64
        self.fns = {stem: getattr(self.lib, "odil_stencil_{}_{}".format(stem, suffix))
                    for stem in ("var_coarsen_batch", "strength_batch", "dense_batch")}

    @staticmethod
    def sizes(shape, halve):
        ndim = len(shape)
        cells = int(np.prod(shape))
        coarse = int(np.prod([n // 2 if h else n for n, h in zip(shape, halve or [1] * ndim)]))
        return (2 * ndim + 1) * cells, (2 * ndim + 1) * coarse

    def coarsen(self, shape=(8, 12), ndim=None, halve=(1, 1), nbatch=3, cs=None, os_=None, null=None):
        need, cneed = self.sizes(shape, halve)
        ptrs = dict(coeffs=c_void_p(4096), coarse=c_void_p(8192), shape=self.i64(shape))
        if null:
            ptrs[null] = None
        mask = None if halve is None else ctypes.cast((c_int * len(halve))(*halve), c_void_p)
        self._keep = mask
        return self.fns["var_coarsen_batch"](
            ptrs["coeffs"], c_int64(need + 3 if cs is None else cs), ptrs["coarse"], c_int64(cneed + 2 if os_ is None else os_),
            ptrs["shape"], c_int(len(shape) if ndim is None else ndim), mask, c_int(nbatch), None)

    def _plain(self, stem, out_name, shape=(8, 12), ndim=None, nbatch=3, cs=None, null=None):
        need, _ = self.sizes(shape, None)
        ptrs = {"coeffs": c_void_p(4096), out_name: c_void_p(8192), "shape": self.i64(shape)}
        if null:
            ptrs[null] = None
        return self.fns[stem](ptrs["coeffs"], c_int64(need + 3 if cs is None else cs), ptrs["shape"],
                              c_int(len(shape) if ndim is None else ndim), c_int(nbatch), ptrs[out_name], None)

    def strength(self, **kw):
        return self._plain("strength_batch", "out", **kw)

    def dense(self, **kw):
        return self._plain("dense_batch", "dense", **kw)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_launchers_refuse_before_launching(suffix):
    """Every refusal: ODIL_E_INVAL and a text that names the entry point and the reason; nothing is launched (with the
    dummy pointers a launch could not succeed)."""
    run = Launchers(suffix)

    def refused(which, text, **kw):
        assert getattr(run, which)(**kw) == -1, (which, kw)
        err = run.lib.odil_last_error()
        name = {"coarsen": b"stencil_var_coarsen_batch", "strength": b"stencil_strength_batch", "dense": b"stencil_dense_batch"}
        assert name[which] in err and text in err, (which, kw, err)

    for which, out in (("coarsen", "coarse"), ("strength", "out"), ("dense", "dense")):
        for null in ("coeffs", out, "shape"):
            refused(which, b"null pointer", null=null)
        refused(which, b"ndim 0", ndim=0)
        refused(which, b"ndim 4", shape=(4, 4, 4, 4), ndim=4)
        refused(which, b"0 members", nbatch=0)
        refused(which, b"65536 members", nbatch=65536)
        refused(which, b"-1 members", nbatch=-1)
        need = Launchers.sizes((8, 12), None)[0]
        refused(which, b"coeff_stride", cs=need - 1)
        refused(which, b"smaller than a member", cs=0)
        refused(which, b"empty extent", shape=(8, 0))
    # the coarse operator: extents of the merged axes even, an axis to merge, room for a coarse member
    refused("coarsen", b"not even", shape=(8, 13))
    refused("coarsen", b"not even", shape=(9, 12), halve=(1, 0))
    refused("coarsen", b"not even", shape=(7,), halve=None)
    refused("coarsen", b"no axis to merge", halve=(0, 0))
    refused("coarsen", b"coarse_stride", os_=Launchers.sizes((8, 12), (1, 1))[1] - 1)
    refused("coarsen", b"coarse_stride", halve=(1, 0), os_=Launchers.sizes((8, 12), (1, 0))[1] - 1)
    # the dense matrix: at most 512 unknowns
    refused("dense", b"513 unknowns", shape=(513,))
    refused("dense", b"576 unknowns", shape=(24, 24))
    refused("dense", b"1024 unknowns", shape=(8, 8, 16))


# --------------------------------------------------------------------------------------- fused.newton_stencil_refusal
def test_newton_stencil_refusal_gives_each_reason():
    from odil_amd import fused

    f64 = torch.float64
    assert "4-D" in fused.newton_stencil_refusal((8,) * 4, f64)
    assert "0-D" in fused.newton_stencil_refusal((), f64)
    assert "4 cells per axis" in fused.newton_stencil_refusal((16, 3), f64)
    assert "4 cells per axis" in fused.newton_stencil_refusal((3,), torch.float32)
    assert "35937 cells are above the limit" in fused.newton_stencil_refusal((33,) * 3, f64)
    assert "65536 cells are above the limit" in fused.newton_stencil_refusal((65536,), f64)
    # no coarsening of a 100 x 100 grid ends below 25 x 25
    assert "coarsest level (25, 25) has 625 unknowns" in fused.newton_stencil_refusal((100, 100), f64)
    assert "dtype" in fused.newton_stencil_refusal((16, 16), torch.float16)


@pytest.mark.parametrize("shape", [(4,), (4, 4), (32, 32, 32), (32768,), (12, 20), (128, 128), (8, 4, 16)], ids=str)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_newton_stencil_refusal_admits(shape, dtype):
    from odil_amd import fused

    assert fused.newton_stencil_refusal(shape, dtype) is None


# ------------------------------------------------------------------------------------------ optimize_newton_ensemble
@pytest.fixture()
def api(monkeypatch):
    """(odil, the diffusion ensemble example) with the process-wide `mod` on CPU tensors: problems and states can be
    built, nothing can be computed."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
    import ensemble

    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    return odil, ensemble


def members(ensemble, specs):
    built = []
    for b, spec in enumerate(specs):
        args = ensemble.parse_args(spec.split() + ["--members", str(len(specs))])
        built.append(ensemble.make_member(args, b))
    args = ensemble.parse_args(specs[0].split())
    args.epoch_start, args.epochs = 0, 2
    return args, [p for p, _ in built], [s for _, s in built]


def snapshot(states):
    return [(s.fields["u"].array.data_ptr(), s.fields["u"].array.clone()) for s in states]


def unchanged(states, before):
    return all(s.fields["u"].array.data_ptr() == p and torch.equal(s.fields["u"].array, a) for s, (p, a) in zip(states, before))


def test_refuses_damping_before_touching_a_state(api):
    odil, ensemble = api
    args, problems, states = members(ensemble, ["--ndim 2 --N 16"] * 3)
    before = snapshot(states)
    for name in ("linsolver_damp", "linsolver_dampdiag"):
        setattr(args, name, 0.1)
        with pytest.raises(ValueError, match="optimize_newton_ensemble: damping"):
            odil.util.optimize_newton_ensemble(args, problems, states)
        setattr(args, name, 0)
    assert unchanged(states, before)


@pytest.mark.parametrize("specs,member,reason", [
    (["--ndim 2 --N 16", "--ndim 2 --N 16", "--ndim 2 --N 32"], 2, "cells .* differ from member 0"),
    (["--ndim 2 --N 16 --beta 1", "--ndim 1 --N 16 --beta 1"], 1, "cells .* differ from member 0"),
    (["--ndim 2 --N 16", "--ndim 2 --N 16 --double 0"], 1, "dtype"),
    (["--ndim 2 --N 16", "--ndim 3 --N 33"], 1, "35937 cells are above the limit"),
    (["--ndim 2 --N 16", "--ndim 2 --N 16 --multigrid 1"], 1, "MultigridField .*no multigrid decomposition"),
], ids=["mixed-size", "mixed-ndim", "mixed-dtype", "above-limit", "multigrid-member"])
def test_names_the_first_offending_member(api, specs, member, reason):
    """From the shapes alone: ValueError with the member's index, no operator probed (so no device needed), no state
    touched."""
    odil, ensemble = api
    args, problems, states = members(ensemble, specs)
    before = snapshot(states) if "--multigrid 1" not in specs[-1] else None
    with pytest.raises(ValueError, match="optimize_newton_ensemble: member {}: .*{}".format(member, reason)):
        odil.util.optimize_newton_ensemble(args, problems, states)
    assert before is None or unchanged(states, before)
