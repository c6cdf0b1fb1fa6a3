"""Two smoothing sweeps per pass in the batched cycle of a Newton ensemble, what needs no device: the exported symbols of
odil_stencil_var_smooth2_batch, its refusals (ODIL_E_INVAL before any launch, the pointers are dummies), the launch plan of
a list of sweeps (`gmg.sweep_plan`) and the levels that pair (`gmg.EnsembleLaunchGMG.pair_eligible`)."""

import ctypes
import math
from ctypes import c_int, c_int64, c_void_p

import pytest

NAMES = ["odil_stencil_var_smooth2_batch_f64", "odil_stencil_var_smooth2_batch_f32"]


def test_the_batched_pair_is_exported_with_16_arguments():
    from odil_amd import _lib

    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is c_int and len(fn.argtypes) == 16, (name, fn.argtypes)


class Launcher:
    """The entry point with dummy pointers; every keyword replaces one well-formed argument."""

    P = dict(coeffs=4096, x=8192, b=12288, out=16384, active=20480)

    def __init__(self, suffix):
        from odil_amd import _lib

        self.lib, self.i64 = _lib.load(), _lib.i64
        self.real = ctypes.c_double if suffix == "f64" else ctypes.c_float
        self.fn = getattr(self.lib, "odil_stencil_var_smooth2_batch_" + suffix)

    def __call__(self, shape=(8, 12), ndim=None, nbatch=3, cs=None, xs=None, bs=None, os_=None, null=(), same=False):
        cells = math.prod(shape)
        p = {k: (None if k in null else c_void_p(v)) for k, v in self.P.items()}
        if same:
            p["out"] = p["x"]
        return self.fn(p["coeffs"], c_int64((2 * len(shape) + 1) * cells + 2 if cs is None else cs), p["x"],
                       c_int64(cells if xs is None else xs), p["b"], c_int64(cells if bs is None else bs), p["out"],
                       c_int64(cells if os_ is None else os_), None if "shape" in null else self.i64(shape or [1]),
                       c_int(len(shape) if ndim is None else ndim), c_int(nbatch), self.real(0.9), self.real(0.6), c_int(0),
                       p["active"], None)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_the_batched_pair_refuses_before_launching(suffix):
    run = Launcher(suffix)

    def refused(text, **kw):
        assert run(**kw) == -1, kw  # ODIL_E_INVAL
        err = run.lib.odil_last_error()
        assert b"stencil_var_smooth2_batch" in err and text in err, (kw, err)

    cells = 96
    # what the single pair refuses
    refused(b"ndim=0", ndim=0)
    refused(b"ndim=4", shape=(4, 4, 4, 4), ndim=4)
    refused(b"null shape", null=("shape",))
    refused(b"multiple of 2", shape=(8, 13))
    refused(b"multiple of 2", shape=(7,))
    refused(b"must be >= 2", shape=(1, 12))
    refused(b"must be >= 2", shape=(4, 1, 8))
    # the members
    refused(b"0 members", nbatch=0)
    refused(b"65536 members", nbatch=65536)
    refused(b"too many cells per member", shape=(4096, 8192))
    # strides: a member fits, and begins on a pack of two cells
    refused(b"coeff_stride", cs=5 * cells - 2)
    refused(b"x_stride", xs=cells - 2)
    refused(b"b_stride", bs=cells - 2)
    refused(b"out_stride", os_=cells - 2)
    for name, kw in (("coeff", dict(cs=5 * cells + 1)), ("x", dict(xs=cells + 1)), ("b", dict(bs=cells + 1)),
                     ("out", dict(os_=cells + 1))):
        refused(name.encode() + b"_stride", **kw)
        assert b"odd" in run.lib.odil_last_error(), name
    # pointers
    for null in ("coeffs", "b", "out"):
        refused(b"null pointer", null=(null,))
    refused(b"in-place", same=True)


W = [0.9, 0.6, 0.5, 0.4]


def test_sweep_plan_pairs_from_the_front():
    from odil_amd.gmg import sweep_plan

    assert sweep_plan(W[:1]) == [(0.9,)]
    assert sweep_plan(W[:2]) == [(0.9, 0.6)]
    assert sweep_plan(W[:3]) == [(0.9, 0.6), (0.5,)]
    assert sweep_plan(W[:4]) == [(0.9, 0.6), (0.5, 0.4)]
    assert sweep_plan(W[:3], first_single=False) == sweep_plan(W[:3])
    assert sweep_plan([]) == [] and sweep_plan([], first_single=True) == []


def test_sweep_plan_keeps_the_first_sweep_single():
    from odil_amd.gmg import sweep_plan

    assert sweep_plan(W[:1], first_single=True) == [(0.9,)]
    assert sweep_plan(W[:2], first_single=True) == [(0.9,), (0.6,)]
    assert sweep_plan(W[:3], first_single=True) == [(0.9,), (0.6, 0.5)]
    assert sweep_plan(W[:4], first_single=True) == [(0.9,), (0.6, 0.5), (0.4,)]


@pytest.mark.parametrize("first_single", [False, True])
@pytest.mark.parametrize("n", range(0, 8))
def test_sweep_plan_keeps_the_order_of_the_weights(n, first_single):
    from odil_amd.gmg import sweep_plan

    weights = [1.0 / (k + 2) for k in range(n)]
    plan = sweep_plan(weights, first_single)
    assert [w for launch in plan for w in launch] == weights
    assert all(len(launch) in (1, 2) for launch in plan)
    assert sweep_plan(tuple(weights), first_single) == plan and len(weights) == n  # (any sequence; the input is left alone)


def levels(shapes, nbatch, pair_min_cells=None):
    """An EnsembleLaunchGMG as far as `pair_eligible` looks at it (no device)."""
    from odil_amd.gmg import EnsembleLaunchGMG

    ens = object.__new__(EnsembleLaunchGMG)
    ens.shapes, ens.nbatch = shapes, nbatch
    if pair_min_cells is not None:
        ens.pair_min_cells = pair_min_cells
    return ens


def test_pair_eligible_is_host_arithmetic():
    from odil_amd.gmg import EnsembleLaunchGMG

    shapes = [(64, 64, 64), (32, 32, 32), (16, 16, 16)]
    # never and always
    assert not any(levels(shapes, 4, math.inf).pair_eligible(l) for l in range(3))
    assert all(levels(shapes, 4, 0).pair_eligible(l) for l in range(3))
    assert all(levels(shapes, 1, 0).pair_eligible(l) for l in range(3))
    # an odd last extent never pairs, whatever the threshold; neither does an extent of 1
    odd = [(20, 10), (10, 5), (12, 7, 9), (1, 8)]
    assert [levels(odd, 64, 0).pair_eligible(l) for l in range(4)] == [True, False, False, False]
    # the threshold looks at the cells of ALL members on the level
    assert levels(shapes, 4, 2 ** 20).pair_eligible(0) and not levels(shapes, 1, 2 ** 20).pair_eligible(0)
    assert not levels(shapes, 4, 2 ** 20).pair_eligible(1) and levels(shapes, 32, 2 ** 20).pair_eligible(1)
    assert levels(shapes, 3, 3 * 64 ** 3).pair_eligible(0) and not levels(shapes, 3, 3 * 64 ** 3 + 1).pair_eligible(0)
    # a class attribute, overridable per instance
    one = levels(shapes, 4)
    assert one.pair_min_cells == EnsembleLaunchGMG.pair_min_cells
    one.pair_min_cells = 0
    assert one.pair_eligible(2) and "pair_min_cells" not in vars(levels(shapes, 4))


def test_the_example_takes_a_pair_threshold():
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
    import ensemble

    assert ensemble.parse_args([]).pair_min_cells is None  # (the class's default)
    assert ensemble.parse_args(["--pair_min_cells", "0"]).pair_min_cells == 0
    assert ensemble.parse_args(["--pair_min_cells", "-1"]).pair_min_cells == -1
    assert ensemble.parse_args(["--pair_min_cells", "1048576", "--form", "launches"]).pair_min_cells == 1 << 20
