"""Newton steps for ensembles of Poisson problems on the device: odil_stencil_solve_batch (one workgroup per member runs a
whole multigrid solve), gmg.EnsembleGMG and util.optimize_newton_ensemble.

A  bit pins: with tol = 0 and maxcycles = k member b's iterate equals k single launches of ops.stencil_vcycle_tail on that
   member's arrays alone -- shared Poisson operators and per-member variable-coefficient operators, f64 and f32
B  members do not interact: a member computes the same bits inside a batch and alone; canaries between the members stay
C  the norms of the history against NumPy float64
D  convergence to 1e-10 against the float64 oracle residual and against the cycle count of gmg.PoissonGMG.solve
E  mode 1 (the Newton step) against the oracle's direct solve of the normal equations
F  util.optimize_newton_ensemble against the oracle and against single optimize_newton runs, f64 and f32"""

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
POISSON_SHAPES = [(64,), (12, 20), (40, 40), (8, 4, 16), (16, 16, 16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def spacing2(shape):
    """Equal spacing on every axis: the box is 1 along the longest axis."""
    return [(1.0 / max(shape)) ** 2] * len(shape)


def padded(nb, shape, pad, dtype, dev, fill=CANARY):
    """([nb, *shape] view with `pad` extra elements after every member, the flat [nb, cells + pad] base)."""
    cells = math.prod(shape)
    base = torch.full((nb, cells + pad), fill, dtype=dtype, device=dev)
    strides = [math.prod(shape[k + 1:]) for k in range(len(shape))]
    return base.as_strided((nb,) + tuple(shape), [cells + pad] + strides), base


def pads_intact(base, pad):
    return bool((base[:, -pad:] == CANARY).all())


def random_members(nb, shape, dtype, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((nb,) + tuple(shape), generator=gen, dtype=torch.float64).to(dtype).to(dev)


_ensembles = dict()


def poisson_ensemble(shape, dtype, dev, nb):
    from odil_amd import gmg

    key = (shape, dtype, nb)
    if key not in _ensembles:
        _ensembles[key] = gmg.EnsembleGMG(shape, spacing2(shape), dtype, dev, nb)
    return _ensembles[key]


def single_launch_reference(ens, member, b, x0, ks=(0, 1, 3)):
    """{(start, k): iterate} of ONE member by single launches of the existing one-workgroup cycle on its arrays alone."""
    from odil_amd import ops

    coeffs = ens.coeffs if ens.coeffs.dim() == 1 else ens.coeffs[member]
    inv = ens.inv if ens.inv.dim() == 2 else ens.inv[member]
    work = torch.empty(3 * sum(math.prod(s) for s in ens.shapes), dtype=ens.dtype, device=b.device)
    launch = ops.stencil_vcycle_tail_plan(coeffs.contiguous(), ens.shapes, ens.halve, work, inv.contiguous(), ens.wpre, ens.wpost)
    b = b.contiguous()
    out = dict()
    for start in (0, 1, 2):
        if start == 0:
            x, zero = torch.zeros_like(b), True
        elif start == 1:
            x, zero = x0.clone(), False
        else:
            x, zero = launch(None, b, torch.empty_like(b), fmg=True), False
        for k in range(max(ks) + 1):
            if k in ks:
                out[(start, k)] = x.clone()
            x = launch(None if zero else x, b, torch.empty_like(b))
            zero = False
    return out


_references = dict()


def poisson_reference(shape, dtype, dev, nmax):
    """The single-launch iterates of `nmax` members of a shape, computed once and shared by every batch size."""
    key = (shape, dtype)
    if key not in _references:
        ens = poisson_ensemble(shape, dtype, dev, 1)
        b = random_members(nmax, shape, dtype, dev, 11)
        x0 = random_members(nmax, shape, dtype, dev, 12)
        _references[key] = (b, x0, [single_launch_reference(ens, 0, b[m], x0[m]) for m in range(nmax)])
    b, x0, refs = _references[key]
    assert len(refs) >= nmax
    return b, x0, refs


def check_bit_pins(ens, b, x0, refs, dev, ks=(0, 1, 3)):
    nb, shape = ens.nbatch, ens.shapes[0]
    bp, _ = padded(nb, shape, 5, ens.dtype, dev)
    bp.copy_(b[:nb])
    for start in (0, 1, 2):
        for k in ks:
            x, base = padded(nb, shape, 3, ens.dtype, dev)
            x.copy_(x0[:nb])
            ens.solve(bp, x, tol=0.0, maxcycles=k, start=start)
            assert pads_intact(base, 3), "padding between members was written"
            for m in range(nb):
                assert torch.equal(x[m], refs[m][(start, k)]), (start, k, m)
            assert (ens.outcome[:, 0] == k).all() and (ens.outcome[:, 1] == 1).all(), (start, k, ens.outcome)


# ------------------------------------------------------------------------------------------------------- A: bit pins
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nb", [1, 3, 70])
@pytest.mark.parametrize("shape", POISSON_SHAPES, ids=str)
def test_members_equal_single_launches_bit_for_bit(dev, shape, nb, dtype):
    b, x0, refs = poisson_reference(shape, dtype, dev, 70)
    check_bit_pins(poisson_ensemble(shape, dtype, dev, nb), b, x0, refs, dev)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,nb", [((32, 32, 32), 2), ((8, 8), 300)], ids=["32^3-B2", "8^2-B300"])
def test_largest_member_and_more_workgroups_than_compute_units(dev, shape, nb, dtype):
    b, x0, refs = poisson_reference(shape, dtype, dev, nb)
    check_bit_pins(poisson_ensemble(shape, dtype, dev, nb), b, x0, refs, dev)


def diffusion_coeffs(shape, rng, periodic=None):
    """-div(k grad u) + r u with a smooth positive conductivity (1 : 20), face conductivities by averaging, zero-Dirichlet
    walls at half a cell or one periodic axis, in the layout of the Jacobian's coefficient arrays (0, -e_0, +e_0, ...)."""
    nd = len(shape)
    grids = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
    k = 1.0 + 19.0 * np.prod([np.sin(np.pi * g * rng.integers(1, 3)) ** 2 for g in grids], axis=0)
    off, diag = [], rng.uniform(0.0, 1.0, shape)
    for a in range(nd):
        h2 = (1.0 / shape[a]) ** 2
        km = 0.5 * (k + np.roll(k, 1, axis=a)) / h2
        kp = 0.5 * (k + np.roll(k, -1, axis=a)) / h2
        idx = np.arange(shape[a]).reshape([-1 if j == a else 1 for j in range(nd)])
        if periodic != a:
            diag = diag + np.where(idx == 0, 2.0 * k / h2, km) + np.where(idx == shape[a] - 1, 2.0 * k / h2, kp)
            km, kp = np.where(idx == 0, 0.0, km), np.where(idx == shape[a] - 1, 0.0, kp)
        else:
            diag = diag + km + kp
        off += [-km, -kp]
    return [diag] + off


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,periodic", [((16, 16), None), ((16, 16, 16), 0)], ids=["16^2", "16^3-periodic"])
def test_per_member_operators_equal_single_launches(dev, shape, periodic, dtype):
    """Three members with their own variable-coefficient operators and coarsest inverses (coeff_stride, inv_stride != 0)."""
    from odil_amd import gmg

    rng = np.random.default_rng(5)
    hierarchies = [gmg.StencilGMG(torch.tensor(np.stack(diffusion_coeffs(shape, rng, periodic)), dtype=dtype, device=dev))
                   for _ in range(3)]
    ens = gmg.EnsembleGMG(hierarchies)
    assert ens.coeffs.dim() == 2 and ens.inv.dim() == 3 and ens.nbatch == 3
    assert not torch.equal(ens.coeffs[0], ens.coeffs[1]) and not torch.equal(ens.inv[0], ens.inv[2])
    b = random_members(3, shape, dtype, dev, 21)
    x0 = random_members(3, shape, dtype, dev, 22)
    refs = [single_launch_reference(ens, m, b[m], x0[m]) for m in range(3)]
    check_bit_pins(ens, b, x0, refs, dev)


# -------------------------------------------------------------------------------------- B: members do not interact
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode,start", [(0, 2), (0, 1), (1, 2), (1, 0)], ids=["solve-nested", "solve-x", "newton-nested", "newton-zero"])
def test_a_member_computes_the_same_inside_a_batch_and_alone(dev, dtype, mode, start):
    """Member b's x, history and outcome are the same bits in a batch of 5 and as nbatch = 1 on its own arrays; the canaries
    between the members' x, work, history and outcome records, and after the last, stay."""
    from odil_amd import ops

    shape, nb, maxc, pad = (12, 20), 5, 12, 4
    tol = 1e-10 if dtype == F64 else 1e-5
    ens = poisson_ensemble(shape, dtype, dev, 1)
    need = ops.stencil_solve_batch_work(ens.shapes)
    b = random_members(nb, shape, dtype, dev, 31)
    x0 = random_members(nb, shape, dtype, dev, 32)

    def run(members):
        n = len(members)
        x, xbase = padded(n, shape, pad, dtype, dev)
        x.copy_(x0[members])
        bp, _ = padded(n, shape, pad + 1, dtype, dev)
        bp.copy_(b[members])
        work = torch.full((n, need + pad), CANARY, dtype=dtype, device=dev)
        history = torch.full((n, maxc + 2 + pad), CANARY, dtype=F64, device=dev)
        outcome = torch.full((n + 1, 2), 777, dtype=torch.int32, device=dev)
        plan = ops.stencil_solve_batch_plan(ens.coeffs, ens.shapes, ens.halve, n, work, ens.inv, ens.wpre, ens.wpost)
        plan(x, bp, history, outcome[:n], start, mode, maxc, tol)
        assert pads_intact(xbase, pad) and pads_intact(work, pad), "padding between members was written"
        assert bool((outcome[n] == 777).all())
        return x.clone(), history.cpu().numpy(), outcome[:n].cpu().numpy()

    x, history, outcome = run(list(range(nb)))
    for m in range(nb):
        k = int(outcome[m, 0])
        assert (history[m, 2 + k:] == CANARY).all() and (history[m, :2 + k] != CANARY).all(), (m, k, history[m])
        xa, ha, oa = run([m])
        assert torch.equal(xa[0], x[m]), m
        assert np.array_equal(ha[0], history[m]) and np.array_equal(oa[0], outcome[m]), (m, ha[0], history[m])
    if dtype == F64 and start == 2:
        assert (outcome[:, 1] == 0).all(), outcome


# ---------------------------------------------------------------------------------------------------------- C: norms
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(40, 40), (16, 16, 16), (64,)], ids=str)
def test_history_norms_against_numpy(dev, shape, dtype):
    """history[0] = mean(b^2) (the squares of floats are exact in double; the sums differ by their order only), and from
    the zero start history[1] = mean((A 0 - b)^2) is the same number."""
    nb = 3
    ens = poisson_ensemble(shape, dtype, dev, nb)
    b = random_members(nb, shape, dtype, dev, 41)
    for start in (0, 2):
        x = torch.zeros_like(b)
        ens.solve(b, x, tol=0.0, maxcycles=0, start=start)
        for m in range(nb):
            want = np.mean(b[m].cpu().numpy().astype(np.float64) ** 2)
            got = ens.history[m]
            print("mean(b^2)", shape, dtype, m, got[0], want)
            assert abs(got[0] - want) <= 1e-13 * want
            if start == 0:
                assert abs(got[1] - want) <= 1e-13 * want
                assert not x[m].any()


# ---------------------------------------------------------------------------------------------------- D: convergence
@pytest.mark.parametrize("shape,nb", [(s, 3) for s in POISSON_SHAPES] + [((32, 32, 32), 2)], ids=str)
def test_converges_to_the_tolerance_in_float64(dev, shape, nb):
    from odil_amd import gmg
    from oracle import odil_np as onp

    tol = 1e-10
    h2 = spacing2(shape)
    ens = poisson_ensemble(shape, F64, dev, nb)
    b = random_members(nb, shape, F64, dev, 51)
    x = torch.zeros_like(b)
    ens.solve(b, x, tol=tol, maxcycles=60, start=2)
    single = gmg.PoissonGMG(shape, h2, F64, dev)
    dw = [math.sqrt(v) for v in h2]
    for m in range(nb):
        st = ens.status(m)
        assert ens.outcome[m, 1] == 0 and st["converged"] and not st["stagnated"], (m, st)
        bm = b[m].cpu().numpy()
        rel = np.linalg.norm(onp.poisson_residual(x[m].cpu().numpy(), bm, dw)) / np.linalg.norm(bm)
        ref = dict()
        single.solve(b[m].contiguous(), tol=tol, krylov="never", status=ref)
        print("converged", shape, m, "cycles", st["niter"], "PoissonGMG", ref["niter"], "relative residual", rel)
        assert rel <= 2 * tol, (m, rel)
        assert ref["converged"] and st["niter"] <= ref["niter"] + 2, (m, st["niter"], ref["niter"])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("start", [0, 2])
def test_zero_right_hand_side(dev, start, dtype):
    shape, nb = (12, 20), 3
    ens = poisson_ensemble(shape, dtype, dev, nb)
    b = random_members(nb, shape, dtype, dev, 61)
    b[1].zero_()
    x = random_members(nb, shape, dtype, dev, 62)
    ens.solve(b, x, tol=1e-10 if dtype == F64 else 1e-5, maxcycles=60, start=start)
    assert not x[1].any() and bool(torch.isfinite(x).all())
    assert tuple(ens.outcome[1]) == (0, 0) and ens.history[1, 0] == 0.0 and ens.history[1, 1] == 0.0
    assert ens.status(1)["converged"] and ens.outcome[0, 1] == 0 and ens.outcome[2, 1] == 0


# --------------------------------------------------------------------------------------------------------- E: mode 1
def dense_poisson(shape, dw):
    from oracle import odil_np as onp

    _, matrix = onp.poisson_linearize(np.zeros(shape), np.zeros(shape), dw)
    return matrix.toarray()


@pytest.mark.parametrize("shape", [(64,), (12, 20), (8, 4, 16)], ids=str)
def test_newton_step_against_the_oracle(dev, shape):
    """One step from a random u: u - d with the oracle's d; |u_new - u_ref| <= cond(A) tol |d| is what a relative residual
    of tol guarantees (|A^-1| |r| with |r| <= tol |A| |d|), twice that is asserted.  A second step starts at the solution:
    it moves u by no more than that."""
    from oracle import odil_np as onp

    tol, nb = 1e-10, 3
    h2 = spacing2(shape)
    dw = [math.sqrt(v) for v in h2]
    cond = np.linalg.cond(dense_poisson(shape, dw))
    ens = poisson_ensemble(shape, F64, dev, nb)
    rhs = random_members(nb, shape, F64, dev, 71)
    u = random_members(nb, shape, F64, dev, 72)
    u0 = u.clone()
    ens.newton_step(u, rhs, tol=tol, maxcycles=60)
    u1 = u.clone()
    assert (ens.outcome[:, 1] == 0).all(), ens.outcome
    ens.newton_step(u, rhs, tol=tol, maxcycles=60)
    for m in range(nb):
        vector, matrix = onp.poisson_linearize(u0[m].cpu().numpy(), rhs[m].cpu().numpy(), dw)
        d = onp.solve_normal_direct(matrix, vector).reshape(shape)
        want = u0[m].cpu().numpy() - d
        bound = 2 * cond * tol * np.linalg.norm(d)
        err = np.linalg.norm(u1[m].cpu().numpy() - want)
        moved = np.linalg.norm(u[m].cpu().numpy() - u1[m].cpu().numpy())
        print("newton step", shape, m, "cond", cond, "error", err, "second step moved", moved, "bound", bound)
        assert err <= bound and moved <= bound, (m, err, moved, bound)


# ----------------------------------------------------------------------------------------------------- F: public API
def _api():
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    return odil, poisson


def _member(odil, poisson, spec, b, epochs=2):
    """Member b of a sweep over an examples/poisson problem with a plain unknown: its own right-hand side and guess."""
    args = poisson.parse_args(("--multigrid 0 --optimizer newton " + spec).split())
    args.epoch_start, args.epochs = 0, epochs
    problem, state = poisson.make_problem(args)
    domain = problem.domain
    gen = torch.Generator().manual_seed(200 + b)
    rhs = problem.extra.rhs
    problem.extra.rhs = rhs * (1.0 + 0.25 * b) + 0.1 * torch.randn(tuple(rhs.shape), generator=gen, dtype=F64).to(rhs.dtype).to(rhs.device)
    (a,) = domain.arrays_from_state(state)
    domain.arrays_to_state([0.05 * torch.randn(tuple(a.shape), generator=gen, dtype=F64).to(a.dtype).to(a.device)], state)
    return args, problem, state


def _oracle_newton(u0, rhs, dw, epochs):
    from oracle import odil_np as onp

    u, first = u0.astype(np.float64), None
    for _ in range(epochs):
        vector, matrix = onp.poisson_linearize(u, rhs.astype(np.float64), dw)
        d = onp.solve_normal_direct(matrix, vector).reshape(u.shape)
        first = np.linalg.norm(d) if first is None else first
        u = u - d
    return u, first


SPECS = ["--ndim 1 --N 64", "--ndim 2 --N 16", "--ndim 3 --N 8"]


def _run_ensemble(odil, poisson, spec, nb=5):
    built = [_member(odil, poisson, spec, b) for b in range(nb)]
    args, problems, states = built[0][0], [p for _, p, _ in built], [s for _, _, s in built]
    start = [(p.extra.rhs.cpu().numpy().copy(), s.fields["u"].array.cpu().numpy().copy()) for p, s in zip(problems, states)]
    seen = [[] for _ in range(nb)]

    def callback(member, state, epoch, pinfo):
        assert state is states[member]
        seen[member].append((epoch, float(np.array(pinfo["loss"])), pinfo.get("linsolver")))

    arrays, info = odil.util.optimize_newton_ensemble(args, problems, states, callback)
    return args, problems, states, start, seen, arrays, info


@pytest.mark.parametrize("spec", SPECS, ids=["1d-64", "2d-16", "3d-8"])
def test_optimize_newton_ensemble_float64(dev, spec):
    from oracle import odil_np as onp

    odil, poisson = _api()
    nb, tol = 5, 1e-10
    full = spec + " --linsolver multigrid"
    args, problems, states, start, seen, arrays, info = _run_ensemble(odil, poisson, full, nb)
    cshape = tuple(problems[0].domain.cshape)
    dw = onp.step(cshape)
    cond = np.linalg.cond(dense_poisson(cshape, dw))
    assert len(arrays) == nb and info.epochs == 2 and info.cycles.shape == (nb, 2) and info.residuals.shape == (nb, 2)
    packed = info.solver  # (the states alias one packed iterate)
    base = states[0].fields["u"].array.untyped_storage().data_ptr()
    for b in range(nb):
        assert [e for e, _, _ in seen[b]] == [0, 1, 2]
        assert seen[b][0][2] is None and all(st["converged"] and st["method"] == packed.method for _, _, st in seen[b][1:])
        assert info.cycles[b, 0] == seen[b][1][2]["niter"] >= 1
        field = states[b].fields["u"].array
        assert field.untyped_storage().data_ptr() == base and field.storage_offset() == b * math.prod(cshape)
        assert arrays[b][0].data_ptr() == field.data_ptr()
        rhs, u0 = start[b]
        want, dnorm = _oracle_newton(u0, rhs, dw, 2)
        bound = 2 * cond * tol * dnorm
        got = field.cpu().numpy()
        sargs, sproblem, sstate = _member(odil, poisson, full, b)
        odil.util.optimize_newton(sargs, sproblem, sstate)
        alone = sstate.fields["u"].array.cpu().numpy()
        print("api", spec, b, "vs oracle", np.linalg.norm(got - want), "vs optimize_newton", np.linalg.norm(got - alone), "bound", bound)
        assert np.linalg.norm(got - want) <= bound and np.linalg.norm(got - alone) <= bound
        assert seen[b][2][1] <= 1e-12 * max(seen[b][0][1], 1e-300)  # (the loss the callback saw fell to rounding)


def test_optimize_newton_ensemble_direct(dev):
    """`--linsolver direct` asks the cycles for round-off: converged to DIRECT_GMG_TOL, or stopped at the rounding floor."""
    odil, poisson = _api()
    args, problems, states, start, seen, arrays, info = _run_ensemble(odil, poisson, "--ndim 2 --N 16 --linsolver direct", 5)
    for b in range(5):
        for _, _, st in seen[b][1:]:
            assert st["converged"] or st["stagnated"], (b, st)
            if st["converged"]:
                assert st["residual"] <= odil.linsolver.DIRECT_GMG_TOL * st["bnorm"]


@pytest.mark.parametrize("spec", SPECS, ids=["1d-64", "2d-16", "3d-8"])
def test_optimize_newton_ensemble_float32(dev, spec):
    """Both routes stop at the float32 rounding floor: the ensemble's error against the float64 oracle is at most 4 x that
    of the member's single float32 optimize_newton run (operation order)."""
    from oracle import odil_np as onp

    odil, poisson = _api()
    nb = 5
    full = spec + " --linsolver multigrid --double 0"
    args, problems, states, start, seen, arrays, info = _run_ensemble(odil, poisson, full, nb)
    cshape = tuple(problems[0].domain.cshape)
    dw = onp.step(cshape)
    for b in range(nb):
        assert states[b].fields["u"].array.dtype == F32
        rhs, u0 = start[b]
        want, _ = _oracle_newton(u0, rhs, dw, 2)
        sargs, sproblem, sstate = _member(odil, poisson, full, b)
        odil.util.optimize_newton(sargs, sproblem, sstate)
        scale = np.linalg.norm(want)
        err = np.linalg.norm(states[b].fields["u"].array.cpu().numpy() - want) / scale
        alone = np.linalg.norm(sstate.fields["u"].array.cpu().numpy() - want) / scale
        print("api float32", spec, b, "ensemble error", err, "optimize_newton error", alone)
        assert err <= 4 * alone, (b, err, alone)
