"""The multigrid for the normal equations of several grid fields (odil_amd/gmg.py: NormalGMG, csrc/block_mg.hip) on the
GPU: the `multigrid` route of `linsolver.solve` for systems no earlier route takes -- several fields, mixed locations,
non-square or damped M (the reference: AMG on the normal equations + CG, linsolver.py:61-72).

  * the assembled A is M^T M (+ damping) of the dense M; apply is A x; every coarse level is the restatement's P^T A P
    (tests/normal_gmg_np.py): darcy 2-D / 3-D, the uc / ufx operator of the reference's Newton test, veltracer (periodic)
  * the V-cycle is symmetric and positive; solutions match the dense normal-equation solve, damped or not, f32 too
  * darcy 2-D at N = 256, 512, 1024: CG iterations stay flat (measured: 26 at every size; Jacobi CG ends its 1000
    iterations at relative residuals 1e-3 - 1.4 there)
  * through the public API: one Newton step on darcy at 1024^2 and 128^3; veltracer with --linsolver_maxiter 10"""

import importlib
import os
import sys

import normal_gmg_np as ng
import numpy as np
import pytest
import torch
from conftest import ROOT

pytestmark = pytest.mark.gpu


def example(name):
    sub = {"darcy": "darcy", "veltracer": "velocity_from_tracer"}[name]
    p = os.path.join(ROOT, "examples", sub)
    if p not in sys.path:
        sys.path.insert(0, p)
    return importlib.import_module(name)


def uc_ufx_problem(nx=8, ny=4):
    """Cells and x-faces coupled as in the reference's tests/test_newton.py (without its Array and network): the
    x-derivative of ufx, a wall value of ufx, and uc as the mean of the two faces -- M is not square."""
    import odil_amd as odil

    domain = odil.Domain(cshape=(nx, ny), dimnames=["x", "y"], lower=(0, 0), upper=(nx, ny), dtype=np.float64, multigrid=0)
    rng = np.random.default_rng(5)
    dudx = domain.mod.cast(rng.standard_normal((nx, ny)), domain.dtype)

    def operator(ctx):
        mod = ctx.mod
        um, up = ctx.field("ufx", 0, 0, loc="cc"), ctx.field("ufx", 1, 0, loc="cc")
        ufx = ctx.field("ufx")
        wall = mod.where(ctx.indices("x", loc="nc") == 0, ctx.cast(1), ctx.cast(0))
        return [(up - um) / ctx.step("x") - dudx, (ufx - 1.0) * wall, (up + um) * 0.5 - ctx.field("uc")]

    state = odil.State(fields={"uc": odil.Field(None, loc="cc"), "ufx": odil.Field(None, loc="nc")})
    state = domain.init_state(state)
    return odil.Problem(operator, domain), state


def make(name, argv=()):
    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    if name == "uc_ufx":
        return uc_ufx_problem(*argv) if argv else uc_ufx_problem()
    ex = example(name)
    return ex.make_problem(ex.parse_args(list(argv)))


def linearize(name, argv=(), seed=0):
    problem, state = make(name, argv)
    # a state away from zero (veltracer's operator is nonlinear: its upwind switches depend on the velocity)
    rng = np.random.default_rng(seed)
    arrays = [torch.as_tensor(rng.standard_normal(tuple(a.shape)) * 0.1, dtype=a.dtype).to(a.device)
              for a in problem.domain.arrays_from_state(state)]
    problem.domain.arrays_to_state(arrays, state)
    vector, op = problem.linearize_device(state)
    return vector, op


SMALL = [("darcy", ("--ndim", "2", "--N", "8")), ("darcy", ("--ndim", "3", "--N", "4")), ("uc_ufx", ()),
         ("veltracer", ("--Nt", "4", "--Nx", "8", "--multigrid", "0", "--double", "1"))]
IDS = ["darcy2", "darcy3", "uc_ufx", "veltracer-periodic"]


def normal_matrix(op, damp=0.0, dampdiag=0.0):
    m = op.to_dense().double().cpu().numpy()  # (padded reads dropped: the matrix matvec applies)
    a = m.T @ m
    if damp or dampdiag:
        a[np.diag_indices_from(a)] = (np.diag(a) + damp**2) * (1 + dampdiag**2)
    return a


@pytest.mark.parametrize("case", SMALL, ids=IDS)
@pytest.mark.parametrize("damp,dampdiag", [(0.0, 0.0), (0.5, 0.3)])
def test_assembled_operator_and_levels(case, damp, dampdiag):
    from odil_amd import gmg

    _, op = linearize(*case)
    solver = gmg.NormalGMG.create(op, damp, dampdiag)
    assert solver is not None and solver.nlvl >= 2
    want = normal_matrix(op, damp, dampdiag)
    got = solver.dense(0)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # apply
    rng = np.random.default_rng(1)
    for lvl in range(solver.nlvl):
        amat = solver.dense(lvl)
        x = rng.standard_normal(amat.shape[0])
        y = solver.apply(lvl, torch.as_tensor(x, device=op.device)).cpu().numpy()
        assert np.abs(y - amat @ x).max() <= 1e-13 * np.abs(amat).max() * np.abs(x).max() * 8
    # every coarse level is P^T A P of the level above (P of the restatement)
    for lvl in range(1, solver.nlvl):
        kinds = ["".join(".cn"[c] for c in cf) for cf in solver.codes[lvl - 1]]
        p = ng.p_level(solver.shapes[lvl - 1], kinds).toarray()
        ptap = p.T @ solver.dense(lvl - 1) @ p
        assert np.abs(solver.dense(lvl) - ptap).max() <= 1e-13 * np.abs(ptap).max(), lvl


@pytest.mark.parametrize("case", [("darcy", ("--ndim", "2", "--N", "32")), SMALL[3]], ids=["darcy2", "veltracer"])
def test_vcycle_is_symmetric_positive(case):
    from odil_amd import gmg

    _, op = linearize(*case)
    solver = gmg.NormalGMG.create(op, 0.0, 0.0)
    rng = np.random.default_rng(2)
    n = op.ncols
    for _ in range(3):
        u = torch.as_tensor(rng.standard_normal(n), device=op.device)
        v = torch.as_tensor(rng.standard_normal(n), device=op.device)
        bu, bv = solver.precondition(u), solver.precondition(v)
        lhs, rhs = float(u @ bv), float(bu @ v)
        assert abs(lhs - rhs) <= 1e-12 * float(u.norm()) * float(bv.norm()), (lhs, rhs)
        assert float(u @ bu) > 0


@pytest.mark.parametrize("case", SMALL + [("darcy", ("--ndim", "2", "--N", "16", "--double", "0")),
                                          ("darcy", ("--ndim", "2", "--N", "32", "--curl", "0"))],
                         ids=IDS + ["darcy2-f32", "darcy2-square"])
@pytest.mark.parametrize("damp,dampdiag", [(0.0, 0.0), (0.1, 0.0), (0.0, 0.2), (0.3, 0.1)])
def test_route_matches_dense_normal(case, damp, dampdiag):
    import argparse

    import odil_amd as odil

    vector, op = linearize(*case)
    args = argparse.Namespace(linsolver_tol=1e-13, linsolver_maxiter=None, linsolver_damp=damp, linsolver_dampdiag=dampdiag)
    status = dict()
    x = odil.linsolver.solve(op, -vector, args, status, "multigrid")
    assert status["method"].startswith("gmg-normal"), status
    assert x.dtype == op.dtype
    wide = op.promoted() if op.dtype == torch.float32 else op
    ref = odil.linsolver.dense_normal(wide, -vector.double(), damp, dampdiag)
    tol = 1e-9 if op.dtype == torch.float64 else 1e-5
    assert float((x.double() - ref).abs().max()) <= tol * float(ref.abs().max()), status


def darcy_solve(N, tol=1e-8, maxiter=None, ndim=2):
    import argparse

    import odil_amd as odil

    vector, op = linearize("darcy", ("--ndim", str(ndim), "--N", str(N)))
    args = argparse.Namespace(linsolver_tol=tol, linsolver_maxiter=maxiter, linsolver_damp=0, linsolver_dampdiag=0)
    status = dict()
    x = odil.linsolver.solve(op, -vector, args, status, "multigrid")
    return x, status, op, vector


def test_darcy_iterations_stay_flat():
    """Fails without the feature: Jacobi CG on M^T M stops at its 1000-iteration cap far above 1e-8 at these sizes."""
    iters = []
    for N in (256, 512, 1024):
        x, status, op, vector = darcy_solve(N)
        assert status["method"].startswith("gmg-normal") and status["converged"], status
        iters.append(status["niter"])
        res = op.matvec(x) + vector
        assert float(res.norm()) <= 1e-6 * float(vector.norm()), (N, status)
    # (measured 26, 26, 26; the issue's bounds are <= 40 and 1.5x per size: kept with a margin for the read-back every
    # second iteration)
    assert max(iters) <= 34, iters
    assert all(b <= 1.25 * a for a, b in zip(iters, iters[1:])), iters


def test_two_solves_are_bit_identical():
    x1, s1, _, _ = darcy_solve(128)
    x2, s2, _, _ = darcy_solve(128)
    assert s1["niter"] == s2["niter"] and torch.equal(x1, x2)


@pytest.mark.parametrize("argv", [("--ndim", "2", "--N", "1024"), ("--ndim", "3", "--N", "128")], ids=["1024^2", "128^3"])
def test_darcy_newton_step_through_the_api(argv):
    import odil_amd as odil

    ex = example("darcy")
    args = ex.parse_args(list(argv) + ["--linsolver", "multigrid", "--linsolver_tol", "1e-12"])
    odil.util.set_log_file(open(os.devnull, "w"))
    problem, state = ex.make_problem(args)
    loss0 = float(problem.eval_loss_grad(state)[0])
    args.epoch_start, args.epochs = 0, 1
    seen = []
    odil.util.optimize(args, "newton", problem, state, lambda s, e, p: seen.append(p.get("linsolver") if hasattr(p, "get") else None))
    loss1 = float(problem.eval_loss_grad(state)[0])
    st = [s for s in seen if s]
    assert st and st[-1]["method"].startswith("gmg-normal"), st
    assert loss1 <= 1e-14 * loss0, (loss0, loss1, st)
    # the step solved M d = -r: the new residual is at round-off
    vector, op = problem.linearize_device(state)
    assert float(vector.abs().max()) <= 1e-9 * float(problem.extra.f.abs().max()), st


def test_veltracer_newton_step_takes_the_route():
    import odil_amd as odil

    ex = example("veltracer")
    losses = dict()
    for ls in ("direct", "multigrid"):
        args = ex.parse_args(["--Nt", "8", "--Nx", "16", "--multigrid", "0", "--double", "1", "--optimizer", "newton",
                              "--linsolver", ls, "--linsolver_maxiter", "10"])
        odil.util.set_log_file(open(os.devnull, "w"))
        problem, state = ex.make_problem(args)
        args.epoch_start, args.epochs = 0, 1
        seen = []
        odil.util.optimize(args, "newton", problem, state, lambda s, e, p: seen.append(p.get("linsolver") if hasattr(p, "get") else None))
        st = [s for s in seen if s]
        losses[ls] = (float(problem.eval_loss_grad(state)[0]), st[-1] if st else None)
    assert losses["multigrid"][1]["method"].startswith("gmg-normal"), losses
    assert losses["direct"][1]["method"].startswith("dense"), losses
    assert losses["multigrid"][0] <= losses["direct"][0] * (1 + 1e-6) + 1e-12, losses
