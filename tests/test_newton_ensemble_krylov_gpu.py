"""The hand-over to GCR inside the one-launch Newton solve of an ensemble (odil_stencil_solve_krylov_batch,
gmg.EnsembleGMG(krylov="auto"), util.optimize_newton_ensemble(krylov="auto")) on the device.  Members that never meet the
hand-over rule keep every bit of krylov="never"; convection-dominated members that "never" loses are solved, reported with
the cycle of the hand-over, and held to a float64 residual formed on the host (float32: to the error of the member's single
`StencilGMG.solve(krylov="auto")` run against the dense float64 solution).  The facts the cases rest on -- which members
plain cycles lose within the budget, that GCR brings them in, that the members of a case share their levels -- are asserted
in the NumPy model by tests/test_newton_ensemble_krylov_host.py.

The budgets K (model.CASE_A / CASE_B) come from the single run `gmg.StencilGMG.solve` on the hard member of each case --
the reference, not the code under test -- measured on an MI355X in float64 at tol 1e-10 (in brackets: the NumPy model of
tests/ensemble_krylov_np.py, which starts from zero, smooths with other weights and has no second cycle on level 1):
    case A, 1-D 64, v = 200, K = 60:  krylov="auto" 26 passes [26];  krylov="never" stops after 3 cycles, the residual
                                      growing (relative residual 2e2) [3, stagnated]: not converged
    case B, 8^3,   v = 800, K = 40:   krylov="auto" 29 passes [27];  krylov="never" not converged after 1.3 K = 52 cycles
                                      (relative residual 9e-7) [not at 40]
so the single run needs at most K / 1.3 passes (46 and 30.8) with "auto" and is not converged at 1.3 K cycles with "never"
(`test_the_single_runs_set_the_budgets` holds it to that).  The ensemble itself took 29 passes on the member of case A and
27 on that of case B (hand-over before cycle 2 in both), 16 on case B's v = 200 member, which "never" brings in at cycle 40.

In float32 (tolerance 50 eps = 6e-6) the single run on case B's v = 800 member takes 16 passes with "auto" and converges
with "never" only in cycle 45: K = 40 would let "never" pass, so float32 runs case B -- and the 8^3 members of the public
API cases, which "never" brings in after 38 cycles in float32 -- with K_B32 = 24 (24 / 1.3 = 18.5 >= 16, 1.3 x 24 = 32 < 45).
Case A keeps K = 60 in float32: 16 passes with "auto", and "never" stops after 3 cycles as in float64.

The right-hand sides are b = A u of a rough u (model.case_arrays says why: a float32 floor below the tolerance).  The benign
random members have the conductivity 1 : 2 -- at the 1 : 20 of tests/test_newton_ensemble_stencil_gpu.py the plain cycles
lose the 1-D and 2-D members (in the model; seen on the device for 1-D float64) and GCR brings them in: no benign members."""

import math
import os
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT

import ensemble_krylov_np as model
import stencil_gmg_np as sg

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DTYPES = [F64, F32]
DTYPE_IDS = ["f64", "f32"]
TOL = 1e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def tolerance(dtype):
    """The driver's: at least 50 eps of the working precision."""
    return max(TOL, 50 * float(torch.finfo(dtype).eps))


benign_members, case_arrays, CASE_A, CASE_B, CASES = (model.benign_members, model.case_arrays, model.CASE_A, model.CASE_B,
                                                           model.CASES)
K_A, K_B = CASE_A[2], CASE_B[2]
K_B32 = 24


def budget_of(case, dtype):
    """The cycle budget of a case: the model's (float64), and K_B32 for case B in float32, whose tolerance of 50 eps
    plain cycles reach in fewer cycles -- set by the same rule from the single run in float32 (module docstring)."""
    return K_B32 if case[0] == "B" and dtype == F32 else case[2]



def launch(coeffs, b, dtype, dev, krylov, maxcycles, mode="solve", x0=None):
    """(x, history, outcome, [status]) of one launch on members `coeffs` / `b` (NumPy float64) in `dtype`."""
    from odil_amd import gmg

    ct = torch.tensor(coeffs, dtype=dtype, device=dev)
    bt = torch.tensor(b, dtype=dtype, device=dev)
    ens = gmg.EnsembleGMG.from_coeffs(ct, krylov=krylov)
    x = torch.zeros_like(bt) if x0 is None else torch.tensor(x0, dtype=dtype, device=dev)
    getattr(ens, mode)(*((bt, x) if mode == "solve" else (x, bt)), tol=tolerance(dtype), maxcycles=maxcycles)
    torch.cuda.synchronize()
    return x, ens.history.copy(), ens.outcome.copy(), [ens.status(m) for m in range(ct.shape[0])], ens


# ------------------------------------------------------------------------------------- 1: benign members, nothing changes
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", [(64,), (16, 16), (8, 8, 8)], ids=["64", "16x16", "8^3"])
def test_benign_members_keep_every_bit(dev, shape, dtype):
    coeffs = benign_members(shape, 3)
    rng = np.random.default_rng(11)
    b = np.stack([sg.apply(list(c), rng.standard_normal(shape)) for c in coeffs])  # (a rough solution: model.case_arrays)
    u0 = rng.standard_normal((3,) + shape)
    for mode, x0 in (("solve", None), ("newton_step", u0)):
        xn, hn, on, sn, _ = launch(coeffs, b, dtype, dev, "never", 60, mode, x0)
        xa, ha, oa, sa, ens = launch(coeffs, b, dtype, dev, "auto", 60, mode, x0)
        assert on.shape == (3, 2) and oa.shape == (3, 3) and ens.krylov == "auto"
        assert torch.equal(xa, xn), (mode, shape)
        assert np.array_equal(ha, hn) and np.array_equal(oa[:, :2], on) and (oa[:, 2] == -1).all()
        for m in range(3):
            assert sa[m]["handover"] is None and sa[m]["converged"] and sa[m]["method"] == sn[m]["method"] == ens.method
            assert sn[m]["handover"] is None
        need = ens.work.shape[1]
        levels = sum(3 * math.prod(s) for s in ens.shapes)
        assert need == levels + 14 * math.prod(shape)


# ------------------------------------------------------------------------- 2, 3: hard members are solved, honestly reported
def dense_matrix(coeffs):
    shape = coeffs[0].shape
    n = coeffs[0].size
    eye = np.eye(n).reshape((n,) + shape)
    return np.stack([sg.apply(list(coeffs), eye[j]).reshape(-1) for j in range(n)], axis=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES, ids=["A-1d-64", "B-8^3"])
def test_hard_members_are_solved_and_reported(dev, case, dtype):
    """float64: the residual formed on the host in float64 from the member's coefficient arrays is at most 2 tol |b| (the
    kernel tests the same quantity in the same precision in another summation order; the rounding of A x, eps |A| |x| / |b|
    <~ 1e-13 here, is what the factor 2 is for).  float32: the error against the dense float64 solution is at most 4 x that
    of the member's single `StencilGMG.solve(krylov="auto")` run (measured, MI355X: 0.10 - 1.7 x on the members that hand
    over, 0.47 x and 0.89 x on the benign ones)."""
    from odil_amd import gmg

    name, shape, _, members, hard, benign = case
    budget = budget_of(case, dtype)
    coeffs, b = case_arrays(case)
    nb = len(members)
    tol = tolerance(dtype)
    _, _, _, never, _ = launch(coeffs, b, dtype, dev, "never", budget)
    x, hist, out, auto, ens = launch(coeffs, b, dtype, dev, "auto", budget)
    # the members walk one set of levels: every member takes member 0's decision on every level (`_decide` raises otherwise)
    for lvl in range(len(ens.shapes) - 1):
        assert ens._decide(ens.level(lvl), lvl, ens.shapes[lvl]) == ens.halve[lvl], lvl
    for m in range(nb):
        print("case", name, dtype, "member", m, members[m][0], "never", never[m]["niter"], never[m]["converged"], "auto",
              auto[m]["niter"], auto[m]["converged"], auto[m]["handover"], "residual", auto[m]["residual"] / auto[m]["bnorm"])
    for m in hard:
        assert not never[m]["converged"], (m, never[m])
        assert auto[m]["handover"] is not None and auto[m]["handover"] >= 2 and auto[m]["method"].endswith(" + GCR(6)")
        assert auto[m]["method"].startswith(ens.method)
    for m in range(nb):
        assert auto[m]["converged"] and auto[m]["niter"] <= budget, (m, auto[m])
        assert auto[m]["handover"] is None or auto[m]["handover"] >= 2
    # members never communicate: a benign member's bits are those of a launch that holds only the benign members
    xb, hb, ob, alone, _ = launch(coeffs[benign], b[benign], dtype, dev, "auto", budget)
    for i, m in enumerate(benign):
        assert auto[m]["handover"] is None and auto[m]["method"] == ens.method
        assert torch.equal(x[m], xb[i]) and np.array_equal(hist[m], hb[i]) and np.array_equal(out[m], ob[i])
    # the operator both precisions see: the coefficient arrays rounded to the working precision
    seen = torch.tensor(coeffs, dtype=dtype).to(F64).numpy()
    bseen = torch.tensor(b, dtype=dtype).to(F64).numpy()
    got = x.to(F64).cpu().numpy()
    for m in range(nb):
        if dtype == F64:
            res = np.linalg.norm(sg.apply(list(seen[m]), got[m]) - bseen[m])
            print("case", name, "member", m, "host residual / (tol |b|)", res / (tol * np.linalg.norm(bseen[m])))
            assert res <= 2 * tol * np.linalg.norm(bseen[m]), (m, res)
        else:
            want = np.linalg.solve(dense_matrix(seen[m]), bseen[m].reshape(-1)).reshape(shape)
            ct = torch.tensor(coeffs[m], dtype=dtype, device=dev)
            status = dict()
            single = gmg.StencilGMG(ct).solve(torch.tensor(b[m], dtype=dtype, device=dev), tol=tol, maxiter=budget,
                                              status=status, krylov="auto")
            err = np.linalg.norm(got[m] - want)
            ref = np.linalg.norm(single.to(F64).cpu().numpy() - want)
            print("case", name, "member", m, "float32 error", err, "single run", ref, status["niter"], status["method"],
                  "ratio", err / ref)
            assert status["converged"] and err <= 4 * ref, (m, err, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_the_restart_of_gcr_is_exercised(dev, dtype):
    """Case A's v = 200 member needs more passes than GCR keeps directions (measured, MI355X: 27 passes after the hand-over
    in float64, 17 in float32 at its tolerance of 50 eps)."""
    coeffs, b = case_arrays(CASE_A)
    _, _, _, auto, _ = launch(coeffs, b, dtype, dev, "auto", K_A)
    st = auto[1]
    print("restart", dtype, "passes", st["niter"], "hand-over", st["handover"])
    assert st["converged"] and st["niter"] - st["handover"] > 6


# -------------------------------------------------------------------------- 4b: a breakdown of GCR ends the member alone
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_preconditioner_that_returns_nothing_is_a_breakdown(dev, dtype):
    """A numerical input, no fault: with no sweeps and an all-zero coarsest inverse the cycle returns its start, so the
    residual stays what it was -- the hand-over rule fires before cycle 2 -- and as the preconditioner of GCR it returns
    e = 0, so |q|^2 = 0: stop reason 4, converged=False, the iterate (zero) untouched and finite.  In the same launch of
    the same operators with their real inverse and sweeps nothing of the kind happens."""
    from odil_amd import gmg, ops

    shape = (16, 16)
    coeffs = benign_members(shape, 2, seed=7)
    rng = np.random.default_rng(4)
    b = np.stack([sg.apply(list(c), rng.standard_normal(shape)) for c in coeffs])
    x, _, out, st, ens = launch(coeffs, b, dtype, dev, "auto", 20)
    assert all(s["converged"] for s in st) and (out[:, 1] == 0).all()
    nothing = ops.stencil_solve_krylov_batch_plan(ens.coeffs, ens.shapes, ens.halve, 2, ens.work, torch.zeros_like(ens.inv),
                                                  [], [], 6)
    bt = torch.tensor(b, dtype=dtype, device=dev)
    x = torch.full_like(bt, 7.0)
    history = torch.zeros((2, 22), dtype=F64, device=dev)
    outcome = torch.full((2, 3), -5, dtype=torch.int32, device=dev)
    nothing(x, bt, history, outcome, 0, 0, 20, tolerance(dtype))
    torch.cuda.synchronize()
    assert outcome.cpu().tolist() == [[2, 4, 2], [2, 4, 2]]
    assert torch.equal(x, torch.zeros_like(x))
    hist = history.cpu().numpy()
    assert (hist[:, 1] == hist[:, 0]).all() and (hist[:, 2] == hist[:, 0]).all() and (hist[:, 3] == hist[:, 0]).all()
    ens.outcome, ens.history = outcome.cpu().numpy(), hist
    status = ens.status(0)
    assert not status["converged"] and not status["stagnated"] and status["handover"] == 2


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_the_single_runs_set_the_budgets(dev, dtype):
    """The reference behind K_A, K_B and K_B32 (module docstring): the single run needs at most K / 1.3 passes with
    krylov="auto" and is not converged at 1.3 K cycles with krylov="never"."""
    from odil_amd import gmg

    for case in CASES:
        name, shape, _, members, hard, _ = case
        budget = budget_of(case, dtype)
        coeffs, b = case_arrays(case)
        for m in hard:
            ct = torch.tensor(coeffs[m], dtype=dtype, device=dev)
            bt = torch.tensor(b[m], dtype=dtype, device=dev)
            auto, never = dict(), dict()
            gmg.StencilGMG(ct).solve(bt, tol=tolerance(dtype), maxiter=budget, status=auto, krylov="auto")
            gmg.StencilGMG(ct).solve(bt, tol=tolerance(dtype), maxiter=math.ceil(1.3 * budget), status=never, krylov="never")
            print("budget", name, dtype, "member", m, "auto", auto["niter"], auto["method"], auto["converged"], "never", never["niter"],
                  never["converged"], never["residual"] / never["bnorm"])
            assert auto["converged"] and auto["niter"] <= budget / 1.3 and "GCR" in auto["method"]
            assert not never["converged"]


# ------------------------------------------------------------------------------ 4: non-finite inputs end the member alone
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_nan_member_ends_alone(dev, dtype):
    shape = (16, 16)
    coeffs = benign_members(shape, 3, seed=7)
    rng = np.random.default_rng(3)
    b = np.stack([sg.apply(list(c), rng.standard_normal(shape)) for c in coeffs])
    bad = b.copy()
    bad[1, 5, 7] = np.nan
    x, hist, out, st, _ = launch(coeffs, bad, dtype, dev, "auto", 60)
    assert out[1, 1] == 3 and not st[1]["converged"] and not st[1]["stagnated"] and st[1]["handover"] is None
    xo, ho, oo, so, _ = launch(coeffs[[0, 2]], b[[0, 2]], dtype, dev, "auto", 60)
    for i, m in enumerate((0, 2)):
        assert st[m]["converged"]
        assert torch.equal(x[m], xo[i]) and np.array_equal(hist[m], ho[i]) and np.array_equal(out[m], oo[i])


# ------------------------------------------------------------------------------------------------------ 5-7: public API
def _api():
    sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
    import ensemble

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    return odil, ensemble


def np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _members(ensemble, spec, nb, epochs):
    built = []
    for m in range(nb):
        args = ensemble.parse_args((spec + " --members {}".format(nb)).split())
        args.epoch_start, args.epochs = 0, epochs
        problem, state = ensemble.make_member(args, m)
        built.append((args, problem, state))
    return built[0][0], [p for _, p, _ in built], [s for _, _, s in built]


def _run(odil, ensemble, spec, nb, epochs, krylov):
    args, problems, states = _members(ensemble, spec, nb, epochs)
    start = [np64(s.fields["u"].array) for s in states]
    seen = [[] for _ in range(nb)]

    def callback(member, state, epoch, pinfo):
        seen[member].append((epoch, pinfo.get("linsolver"), [float(np.array(v)) for v in pinfo["norms"]]))

    arrays, info = odil.util.optimize_newton_ensemble(args, problems, states, callback, krylov=krylov)
    return problems, states, start, seen, info


DOUBLE = [" --double 1", " --double 0"]


def linear_spec(double):
    """8^3, v_b = 800 (b + 1) / 3 = 267, 533, 800: the members semi-coarsen alike (the model: v = 200 ... 800); the cycle
    budget of case B in that precision."""
    return "--ndim 3 --N 8 --kind smooth --velocity 800 --linsolver multigrid --linsolver_maxiter {}{}".format(
        K_B if double.endswith("1") else K_B32, double)


def dense_jacobian(odil, problem, state, u):
    """The dense matrix of the member's linear operator and f(u), from its own `linearize_device`."""
    from odil_amd import gmg

    problem.domain.arrays_to_state([torch.tensor(u, dtype=state.fields["u"].array.dtype,
                                                 device=state.fields["u"].array.device)], state)
    vector, matrix = problem.linearize_device(state)
    coeffs = np64(gmg.recognise_stencil(matrix))
    return dense_matrix(coeffs), np64(vector).reshape(-1)


@pytest.mark.parametrize("double", DOUBLE, ids=DTYPE_IDS)
def test_optimize_newton_ensemble_hands_hard_members_over(dev, double):
    """The dense float64 comparison holds the float64 run only (the bound of the float64 acceptance carried through
    |M^-1|; in float32 the rounding of M d is of the order of the tolerance)."""
    odil, ensemble = _api()
    nb = 3
    LINEAR = linear_spec(double)
    problems, states, start, seen, info = _run(odil, ensemble, LINEAR, nb, 1, "auto")
    assert states[0].fields["u"].array.dtype == (F64 if double.endswith("1") else F32)
    assert info.route == "stencil" and info.form == "workgroup" and info.handover.shape == (nb, 1)
    print("api handover", info.handover[:, 0], "cycles", info.cycles[:, 0])
    assert info.handover[nb - 1, 0] >= 2
    for m in range(nb):
        (epoch0, none, _), (epoch1, st, _) = seen[m]
        assert none is None and st["converged"], (m, st)
        assert (st["handover"] is None) == (info.handover[m, 0] < 0)
        if not double.endswith("1"):
            continue
        got = np64(states[m].fields["u"].array)
        fresh = _members(ensemble, LINEAR, nb, 1)
        dense, f = dense_jacobian(odil, fresh[1][m], fresh[2][m], start[m])
        want = start[m] - np.linalg.solve(dense, f).reshape(start[m].shape)
        # |d - d*| <= |M^-1| |M d - f| <= |M^-1| 2 tol |f|  (the residual bound of the float64 acceptance above)
        bound = np.linalg.norm(np.linalg.inv(dense), 2) * 2 * TOL * np.linalg.norm(f)
        print("api member", m, "error", np.linalg.norm(got - want), "bound", bound)
        assert np.linalg.norm(got - want) <= bound
    _, _, _, seen, info = _run(odil, ensemble, LINEAR, nb, 1, "never")
    assert (info.handover == -1).all() and not seen[nb - 1][1][1]["converged"]


@pytest.mark.parametrize("double", DOUBLE, ids=DTYPE_IDS)
def test_an_all_poisson_ensemble_keeps_route_and_bits(dev, double):
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    results = dict()
    for krylov in ("never", "auto"):
        built = []
        for m in range(3):
            args = poisson.parse_args("--multigrid 0 --optimizer newton --ndim 2 --N 16 --linsolver multigrid".split() + double.split())
            args.epoch_start, args.epochs = 0, 2
            problem, state = poisson.make_problem(args)
            problem.extra.rhs = problem.extra.rhs * (1.0 + 0.25 * m)
            built.append((args, problem, state))
        arrays, info = odil.util.optimize_newton_ensemble(built[0][0], [p for _, p, _ in built], [s for _, _, s in built],
                                                          krylov=krylov)
        assert info.route == "poisson" and info.solver.krylov == krylov and info.solver.coeffs.dim() == 1
        assert info.solver.dtype == (F64 if double.endswith("1") else F32)
        results[krylov] = ([a[0].clone() for a in arrays], info.cycles.copy(), info.handover.copy())
    assert all(torch.equal(a, n) for a, n in zip(results["auto"][0], results["never"][0]))
    assert np.array_equal(results["auto"][1], results["never"][1]) and (results["auto"][2] == -1).all()


@pytest.mark.parametrize("double", DOUBLE, ids=DTYPE_IDS)
def test_nonlinear_members_converge_step_by_step(dev, double):
    """The norms fall from epoch to epoch down to the rounding floor of the residual evaluation in the working precision:
    ~8 d operations per cell on terms of size |c0| |u|, each rounded to eps (the floor of
    tests/test_newton_ensemble_stencil_gpu.py::test_optimize_newton_ensemble_nonlinear_float64, for the norm instead of the
    loss); |c0| <= 2 d k_max N^2 + v N + 3 beta u^2 with k_max = 11, N = 8, v = 800, |u| <= 1.  In float64 the floor (3e-11)
    is below every norm of these three epochs, so there the norms simply decrease."""
    odil, ensemble = _api()
    nb, epochs = 3, 3
    spec = linear_spec(double) + " --beta 1"
    eps = float(torch.finfo(F64 if double.endswith("1") else F32).eps)
    floor = 8 * 2 * eps * (2 * 3 * 11 * 64 + 800 * 8 + 3) * 1.0
    _, _, _, seen, info = _run(odil, ensemble, spec, nb, epochs, "auto")
    assert info.route == "stencil" and (info.handover[nb - 1] >= 2).all()
    for m in range(nb):
        assert [e for e, _, _ in seen[m]] == [0, 1, 2, 3]
        assert all(st["converged"] for _, st, _ in seen[m][1:]), (m, seen[m])
        norms = [n[0] for _, _, n in seen[m]]
        print("nonlinear member", m, "norms", norms, "handover", info.handover[m])
        assert norms[1] < norms[0]
        assert all(after < before or before <= floor for before, after in zip(norms, norms[1:])), (m, norms, floor)
    _, _, _, seen, info = _run(odil, ensemble, spec, nb, 1, "never")
    assert not seen[nb - 1][1][1]["converged"]
