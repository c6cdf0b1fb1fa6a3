"""The batched linearisation of Newton ensembles on the device: `odil.util.linearize_ensemble` (one launch of the generated
`k_jac_batch` per group of members that share a library) and `optimize_newton_ensemble(linearize="batched")`.

The members are examples/diffusion with the amplitude sweep of examples/diffusion/ensemble.py (conductivity 1 + a_b (k - 1)),
on the smallest shapes at which the kernel's index paths differ (1-D; four points per thread; a last extent that is no
multiple of 4: one point per thread; 3-D with an extent of 4; a periodic axis), B in {1, 3, 70}, float64 and float32.
The reference is the member's own `problem.linearize_device(state)` -> `gmg.recognise_stencil` (one launch of `k_jac`, or
autograd with ODIL_TRACE_JAC=0), computed once per member and kept; every comparison is bit for bit.

1  bit pins: values and coefficient arrays of every member, canaries between the members' arrays intact, a member alone
   (B = 1) gives the bits it gives inside a batch, one launch
2  two operator functions with different sources: two launches, the groups partition the members
3  host scalars: an operator that reads a tracer with another value per member; calls at changing states and tracer values
   queued without a synchronise in between -- more of them than the staging ring has slots -- each return their own result
4  ODIL_TRACE_JAC=0: every member linearised on its own, B launches, the same process's `linearize_device`
5  the driver: three Newton epochs with beta = 1, `linearize="batched"` against `"members"`: iterates, cycles, residuals and
   statuses bit for bit; `optinfo.linearize_launches`"""

import argparse
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT

pytestmark = pytest.mark.gpu

CANARY = 777.0
F64, F32 = torch.float64, torch.float32
CASES = [((64,), None), ((12, 20), None), ((6, 10), None), ((8, 4, 16), None), ((16, 16, 16), 1)]
CASE_IDS = ["64", "12x20", "6x10", "8x4x16", "16^3-periodic"]
NMAX = 70


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def diffusion_ensemble():
    """examples/diffusion/ensemble.py under a name of its own: examples/poisson has an `ensemble` module too, and whichever
    is imported first under that name stays in `sys.modules` for every test that follows."""
    name = "diffusion_ensemble_example"
    if name not in sys.modules:
        path = os.path.join(ROOT, "examples", "diffusion")
        if path not in sys.path:
            sys.path.append(path)  # (for its `import diffusion`)
        spec = importlib.util.spec_from_file_location(name, os.path.join(path, "ensemble.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


def _api():
    ensemble = diffusion_ensemble()
    import diffusion

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    return odil, diffusion, ensemble


def _stencil(ctx):
    dirs = range(ctx.domain.ndim)
    st = [ctx.field("u")]
    for i in dirs:
        st.append(ctx.field("u", *[-1 if j == i else 0 for j in dirs]))
        st.append(ctx.field("u", *[1 if j == i else 0 for j in dirs]))
    return st


def operator_periodic(ctx):
    """examples/diffusion/ensemble.py's operator with axis `extra.periodic` closed on itself instead of by walls."""
    import diffusion

    extra, axis = ctx.extra, ctx.extra.periodic
    st = _stencil(ctx)
    walls = [i for i in range(ctx.domain.ndim) if i != axis]
    fu = diffusion.flux_divergence(st, extra.kfaces, walls, ctx.indices(), ctx.size(), ctx.step(), ctx.mod, extra.args.sigma)
    km, kp = extra.kfaces[axis]
    fu = fu + (kp * (st[2 * axis + 2] - st[0]) - km * (st[0] - st[2 * axis + 1])) / ctx.step()[axis] ** 2
    if extra.beta:
        fu = fu - extra.beta * (st[0] * st[0] * st[0])
    return [fu - extra.rhs]


def operator_reaction(ctx):
    """A second operator function, whose generated source differs: the example's with a reaction term."""
    return [diffusion_ensemble().operator(ctx)[0] - 0.5 * ctx.field("u")]


def operator_tracer(ctx):
    """... with a reaction coefficient that is a host scalar: `problem.tracers["gamma"]`."""
    return [diffusion_ensemble().operator(ctx)[0] - ctx.tracers["gamma"] * ctx.field("u")]


def random_field(shape, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=gen, dtype=F64).to(dtype).cuda()


def make_member(shape, periodic, dtype, b, beta=0.5, operator=None, tracers=None):
    """Member b of the sweep on `shape`: conductivity 1 + a_b (k - 1), a_b = (b + 1) / NMAX (whatever the batch it is put
    in), its own right-hand side and state."""
    odil, diffusion, ensemble = _api()
    nd = len(shape)
    npdt = np.float64 if dtype == F64 else np.float32
    domain = odil.Domain(cshape=list(shape), dimnames=["x", "y", "z"][:nd], multigrid=False, dtype=npdt)
    mod = domain.mod
    x1 = [np.asarray(mod.numpy(x), dtype=np.float64) for x in domain.points_1d()]
    step = [float(s) for s in domain.step()]
    amp = (b + 1) / NMAX
    kfaces = []
    for i in range(nd):
        pair = []
        for sign in (-0.5, 0.5):
            xx = np.meshgrid(*[x + (sign * step[i] if j == i else 0.0) for j, x in enumerate(x1)], indexing="ij")
            pair.append(mod.cast(1 + amp * (diffusion.conductivity("smooth", xx) - 1), npdt))
        kfaces.append(tuple(pair))
    state = odil.State()
    state.fields["u"] = None
    state = domain.init_state(state)
    domain.arrays_to_state([0.3 * random_field(shape, dtype, 2000 + b)], state)
    extra = argparse.Namespace(rhs=random_field(shape, dtype, 1000 + b), kfaces=kfaces, beta=float(beta), periodic=periodic,
                               args=argparse.Namespace(sigma=0.0))
    if operator is None:
        operator = ensemble.operator if periodic is None else operator_periodic
    return odil.Problem(operator, domain, extra, tracers=tracers), state


def reference(problem, state):
    """(values, coeffs) of one member on its own: `linearize_device` -> `gmg.recognise_stencil`, as clones."""
    from odil_amd import gmg

    vector, matrix = problem.linearize_device(state)
    coeffs = gmg.recognise_stencil(matrix)
    assert coeffs is not None
    return vector.reshape(tuple(coeffs.shape[1:])).clone(), coeffs.clone()


class Sweep:
    """The NMAX members of one (shape, periodic, dtype) and their references, made when first asked for and kept."""

    def __init__(self, shape, periodic, dtype):
        built = [make_member(shape, periodic, dtype, b) for b in range(NMAX)]
        self.problems, self.states = [p for p, _ in built], [s for _, s in built]
        self._ref = dict()

    def ref(self, b):
        if b not in self._ref:
            self._ref[b] = reference(self.problems[b], self.states[b])
        return self._ref[b]


_sweeps = dict()


def sweep(shape, periodic, dtype):
    key = (shape, periodic, dtype)
    if key not in _sweeps:
        _sweeps[key] = Sweep(shape, periodic, dtype)
    return _sweeps[key]


def padded(nb, inner, pad, dtype, dev):
    """([nb, *inner] view whose members are `pad` canaries apart, the buffer behind it)."""
    need = math.prod(inner)
    base = torch.full((nb, need + pad), CANARY, dtype=dtype, device=dev)
    return base[:, :need].unflatten(1, inner), base


# ----------------------------------------------------------------------------------------------------- 1: bit pins
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nb", [1, 3, NMAX])
@pytest.mark.parametrize("shape,periodic", CASES, ids=CASE_IDS)
def test_batched_linearisation_equals_single_launches(dev, shape, periodic, nb, dtype):
    odil, _, _ = _api()
    sw = sweep(shape, periodic, dtype)
    problems, states = sw.problems[:nb], sw.states[:nb]
    nd = len(shape)
    coeffs, cbase = padded(nb, (2 * nd + 1,) + shape, 7, dtype, dev)
    values, vbase = padded(nb, shape, 5, dtype, dev)
    v, c, info = odil.util.linearize_ensemble(problems, states, coeffs=coeffs, values=values)
    assert v.data_ptr() == values.data_ptr() and c.data_ptr() == coeffs.data_ptr()
    assert info.launches == 1 and info.groups == [list(range(nb))] and info.single == []
    assert bool((cbase[:, (2 * nd + 1) * math.prod(shape):] == CANARY).all()), "padding between the members' coefficients was written"
    assert bool((vbase[:, math.prod(shape):] == CANARY).all()), "padding between the members' values was written"
    for b in range(nb):
        want_v, want_c = sw.ref(b)
        assert torch.equal(values[b], want_v), ("values", b)
        assert torch.equal(coeffs[b], want_c), ("coefficients", b, [bool(torch.equal(coeffs[b, s], want_c[s])) for s in range(2 * nd + 1)])
    # a member alone gives the bits it gives inside the batch (own buffers, allocated by the call)
    m = nb - 1
    v1, c1, info1 = odil.util.linearize_ensemble([problems[m]], [states[m]])
    assert info1.launches == 1 and info1.groups == [[0]] and tuple(c1.shape) == (1, 2 * nd + 1) + shape
    assert torch.equal(v1[0], values[m]) and torch.equal(c1[0], coeffs[m])


def test_repeated_calls_reuse_the_plan(dev):
    odil, _, _ = _api()
    sw = sweep((12, 20), None, F64)
    problems, states = sw.problems[:3], sw.states[:3]
    odil.util.linearize_ensemble(problems, states)
    plan = problems[0]._ensemble_linearizer
    v, c, _ = odil.util.linearize_ensemble(problems, states)
    assert problems[0]._ensemble_linearizer is plan
    for b in range(3):
        assert torch.equal(v[b], sw.ref(b)[0]) and torch.equal(c[b], sw.ref(b)[1])


# ---------------------------------------------------------------------------------------------------- 2: two groups
def test_members_of_two_operator_functions_take_two_launches(dev):
    odil, _, ensemble = _api()
    shape, nb = (12, 20), 6
    built = [make_member(shape, None, F64, b, operator=ensemble.operator if b % 2 == 0 else operator_reaction) for b in range(nb)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    v, c, info = odil.util.linearize_ensemble(problems, states)
    assert info.launches == 2 and info.single == []
    assert sorted(info.groups) == [[0, 2, 4], [1, 3, 5]]
    for b in range(nb):
        want_v, want_c = reference(problems[b], states[b])
        assert torch.equal(v[b], want_v) and torch.equal(c[b], want_c), b
    # (the reaction term is seen: the centre coefficients of neighbouring members differ by more than their conductivities)
    assert float((c[1, 0] - c[0, 0]).abs().min()) > 0.0


# --------------------------------------------------------------------------------------------------- 3: host scalars
def test_members_keep_their_own_host_scalars_across_queued_calls(dev):
    from odil_amd.stencil_bind import JacobianBatch

    odil, _, _ = _api()
    shape, nb, ncalls = (12, 20), 4, JacobianBatch.depth + 2
    built = [make_member(shape, None, F64, b, operator=operator_tracer, tracers=dict(gamma=1.0 + b)) for b in range(nb)]
    problems, first = [p for p, _ in built], [s for _, s in built]
    second = [make_member(shape, None, F64, b + 7)[1] for b in range(nb)]
    gamma = lambda k, b: 1.0 + b + 10.0 * k
    torch.cuda.synchronize()
    got = []
    for k in range(ncalls):  # queued back to back: no synchronise, nothing read back
        for b, problem in enumerate(problems):
            problem.tracers["gamma"] = gamma(k, b)
        v, c, info = odil.util.linearize_ensemble(problems, second if k % 2 else first)
        assert info.launches == 1
        got.append((v, c))
    torch.cuda.synchronize()
    for k, (v, c) in enumerate(got):
        for b, problem in enumerate(problems):
            problem.tracers["gamma"] = gamma(k, b)
            want_v, want_c = reference(problem, (second if k % 2 else first)[b])
            assert torch.equal(v[b], want_v) and torch.equal(c[b], want_c), (k, b)
    # the tracer reaches the kernel per member and per call: the centre coefficient moves by the difference of the gammas
    shift = (got[0][1][:, 0] - got[2][1][:, 0]).mean(dim=(1, 2)).cpu().numpy()
    assert np.allclose(shift, 20.0, rtol=0, atol=1e-9), shift
    alone = (got[0][1][0, 0] - got[0][1][1, 0]).abs().min()
    assert float(alone) > 0.0


# ----------------------------------------------------------------------------------------------- 4: per-member path
def test_without_generated_jacobians_every_member_is_single(dev, monkeypatch):
    odil, _, _ = _api()
    monkeypatch.setenv("ODIL_TRACE_JAC", "0")
    shape, nb = (12, 20), 3
    built = [make_member(shape, None, F64, b) for b in range(nb)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    v, c, info = odil.util.linearize_ensemble(problems, states)
    assert info.launches == nb and info.groups == [] and [b for b, _ in info.single] == list(range(nb))
    assert all("Jacobian" in reason for _, reason in info.single)
    for b in range(nb):
        want_v, want_c = reference(problems[b], states[b])
        assert problems[b]._jac_traced is None, "the reference did not take the autograd evaluation"
        assert torch.equal(v[b], want_v) and torch.equal(c[b], want_c), b


# ---------------------------------------------------------------------------------------------------------- 5: driver
@pytest.mark.parametrize("shape", [(12, 20), (8, 4, 16)], ids=["12x20", "8x4x16"])
def test_driver_batched_equals_members_bit_for_bit(dev, shape):
    odil, _, ensemble = _api()
    nb, epochs = 5, 3
    args = ensemble.parse_args("--ndim {} --N 16 --beta 1 --linsolver multigrid".format(len(shape)).split())
    args.epoch_start, args.epochs = 0, epochs
    runs = dict()
    for how in ("batched", "members"):
        built = [make_member(shape, None, F64, b, beta=1.0) for b in range(nb)]
        problems, states = [p for p, _ in built], [s for _, s in built]
        seen = []
        arrays, info = odil.util.optimize_newton_ensemble(
            args, problems, states, lambda member, state, epoch, pinfo: seen.append(
                (member, epoch, state.fields["u"].array.clone(), pinfo.get("linsolver"))), linearize=how)
        assert info.route == "stencil"
        runs[how] = (arrays, info, seen)
    (a0, i0, s0), (a1, i1, s1) = runs["batched"], runs["members"]
    assert i0.linearize_launches.shape == (epochs,) and (i0.linearize_launches == 1).all(), i0.linearize_launches
    assert (i1.linearize_launches == nb).all(), i1.linearize_launches
    assert i0.linearize_ms is None and i1.linearize_ms is None
    assert np.array_equal(i0.cycles, i1.cycles) and (i0.cycles >= 1).all()
    assert np.array_equal(i0.residuals, i1.residuals)
    assert len(s0) == len(s1) == nb * (epochs + 1)
    for (m0, e0, u0, st0), (m1, e1, u1, st1) in zip(s0, s1):  # every iterate and status on the way
        assert (m0, e0) == (m1, e1) and torch.equal(u0, u1) and st0 == st1, (m0, e0)
    for b in range(nb):
        assert torch.equal(a0[b][0], a1[b][0]), b
        assert not torch.equal(a0[b][0], s0[b][2]), "the member did not move"


def test_driver_times_the_linearisation_on_request(dev):
    odil, _, ensemble = _api()
    args = ensemble.parse_args("--ndim 2 --N 16 --beta 1 --linsolver multigrid".split())
    args.epoch_start, args.epochs = 0, 2
    built = [make_member((12, 20), None, F64, b, beta=1.0) for b in range(3)]
    _, info = odil.util.optimize_newton_ensemble(args, [p for p, _ in built], [s for _, s in built], time_linearize=True)
    assert info.linearize_ms.shape == (2,) and (info.linearize_ms > 0).all()
