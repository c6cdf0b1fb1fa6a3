"""The tiled Poisson residual with the last prolongation fused in (csrc/poisson_synth_tile.hip): fu equals, bit for bit,
odil_interp_add followed by odil_poisson_residual, and the loss keeps every bit the single-launch marching kernel gave
it (tests/golden/residual_synth_loss_bits.json, written by tests/golden/make_golden_residual_synth_loss.py from the
commit before the tiled kernel; the inputs are regenerated from that script's seeds)."""
import functools
import importlib.util
import json
import os
from ctypes import c_double, c_int64, c_size_t

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_residual_synth_loss",
                                               os.path.join(GOLDEN, "make_golden_residual_synth_loss.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "residual_synth_loss_bits.json")) as _f:
    LOSS_BITS = json.load(_f)

CASES = [pytest.param(s, dt, id="{}-{}".format(dt, "x".join(map(str, s)))) for s, dt in gen.cases()]
SMALL = [pytest.param(s, dt, id="{}-{}".format(dt, "x".join(map(str, s))))
         for s in [(2, 2, 2), (3, 9, 33), (6, 17, 70)] for dt in ("float64", "float32")]


@functools.lru_cache(maxsize=1)
def problem(cshape, dtype):
    """Device inputs of a case and, per h2 set, the two-kernel reference fu: computed once, never written to."""
    from odil_amd import ops

    dev = torch.device("cuda:0")
    coarse, w0, rhs = (torch.tensor(a, device=dev) for a in gen.make_inputs(cshape, dtype))
    h2s = [[np.dtype(dtype).type(v) for v in h2] for h2 in gen.H2_SETS]
    u = ops.interp_add(coarse, "ccc", add=w0)
    refs = [ops.poisson_residual(u, rhs, h2)[0] for h2 in h2s]
    return coarse, w0, rhs, h2s, refs


def test_every_case_has_a_recorded_loss():
    want = {gen.key(s, dt, i) for s, dt in gen.cases() for i in range(len(gen.H2_SETS))}
    want |= {gen.key(gen.SLAB_SHAPE, dt, i, slab=True) for dt in ("float64", "float32") for i in range(len(gen.H2_SETS))}
    assert set(LOSS_BITS) == want


@pytest.mark.parametrize("cshape,dtype", CASES)
def test_fu_is_bit_identical_and_loss_keeps_every_bit(cshape, dtype):
    from odil_amd import ops

    coarse, w0, rhs, h2s, refs = problem(cshape, dtype)
    for ih2, (h2, fu_ref) in enumerate(zip(h2s, refs)):
        fu, loss = ops.poisson_residual_synth(coarse, w0, rhs, h2)
        assert torch.equal(fu, fu_ref), ih2
        got, want = float(loss).hex(), LOSS_BITS[gen.key(cshape, dtype, ih2)]
        print(cshape, dtype, ih2, "loss", got, "recorded", want)
        assert got == want, ih2


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_slab_form_loss_keeps_every_bit(dtype):
    """zrange / denom (odil_amd/slab.py): fu of every plane, the loss of the inner planes only."""
    from odil_amd import ops

    cshape = gen.SLAB_SHAPE
    coarse, w0, rhs, h2s, refs = problem(cshape, dtype)
    zrange, denom = gen.slab_args(cshape)
    for ih2, (h2, fu_ref) in enumerate(zip(h2s, refs)):
        fu, loss = ops.poisson_residual_synth(coarse, w0, rhs, h2, zrange=zrange, denom=denom)
        assert torch.equal(fu, fu_ref), ih2
        got, want = float(loss).hex(), LOSS_BITS[gen.key(cshape, dtype, ih2, slab=True)]
        print(cshape, dtype, ih2, "slab loss", got, "recorded", want)
        assert got == want, ih2


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_loss_only_without_fu(dtype):
    """fu == NULL through the C ABI: nothing is stored, the loss is the same."""
    from odil_amd import _lib, ops

    cshape = (3, 9, 33)
    coarse, w0, rhs, h2s, _ = problem(cshape, dtype)
    sums = ops.residual_synth_workspace(w0.device, cshape)
    for ih2, h2 in enumerate(h2s):
        loss = torch.zeros((), dtype=w0.dtype, device=w0.device)
        h2a, h2p = _lib.host_reals(h2, w0.dtype)
        _lib.call("poisson_residual_synth", w0.dtype, _lib.ptr(coarse), _lib.ptr(w0), _lib.ptr(rhs), None,
                  _lib.i64(cshape), h2p, c_int64(0), c_int64(-1), c_double(0.0),
                  _lib.ptr(ops.reduce_workspace(w0.device)), _lib.ptr(sums), c_size_t(sums.numel() * 8), _lib.ptr(loss),
                  _lib.stream_ptr())
        assert float(loss).hex() == LOSS_BITS[gen.key(cshape, dtype, ih2)], ih2


@pytest.mark.parametrize("cshape,dtype", SMALL)
def test_two_calls_give_equal_bits(cshape, dtype):
    from odil_amd import ops

    coarse, w0, rhs, h2s, _ = problem(cshape, dtype)
    for h2 in h2s:
        fu1, loss1 = ops.poisson_residual_synth(coarse, w0, rhs, h2)
        fu2, loss2 = ops.poisson_residual_synth(coarse, w0, rhs, h2)
        assert torch.equal(fu1, fu2) and float(loss1).hex() == float(loss2).hex()


def test_workspace_is_refused_when_too_small():
    """The column sums are the caller's: a short workspace is an error before anything is launched."""
    from odil_amd import _lib, ops

    cshape = (3, 9, 33)
    coarse, w0, rhs, h2s, _ = problem(cshape, "float64")
    need = _lib.load().odil_poisson_residual_synth_workspace_bytes(_lib.i64(cshape))
    assert need == 3 * 9 * 33 * 8  # one z-chunk per coarse plane at this size
    sums = ops.residual_synth_workspace(w0.device, cshape)
    loss = torch.zeros((), dtype=w0.dtype, device=w0.device)
    h2a, h2p = _lib.host_reals(h2s[0], w0.dtype)
    with pytest.raises(_lib.OdilHipError, match="column sums"):
        _lib.call("poisson_residual_synth", w0.dtype, _lib.ptr(coarse), _lib.ptr(w0), _lib.ptr(rhs), None,
                  _lib.i64(cshape), h2p, c_int64(0), c_int64(-1), c_double(0.0),
                  _lib.ptr(ops.reduce_workspace(w0.device)), _lib.ptr(sums), c_size_t(need - 8), _lib.ptr(loss),
                  _lib.stream_ptr())
