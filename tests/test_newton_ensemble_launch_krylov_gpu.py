"""The hand-over to GCR ACROSS the batched launches of a Newton ensemble (gmg.EnsembleLaunchKrylovGMG,
odil_stencil_gcr_*_batch, util.optimize_newton_ensemble(krylov="any")) on the device.  Members that never meet the
hand-over rule keep every bit of `gmg.EnsembleLaunchGMG`; convection-dominated members that the plain batched cycles lose
are solved, reported with the cycle of the hand-over and held to a float64 residual formed on the host (float32: to the
error of the member's single `StencilGMG.solve(krylov="auto")` run against the dense float64 solution); a member's bits
do not depend on what else the launch holds.  Cases, right-hand sides and benign members are those of
tests/ensemble_krylov_np.py (the model describes a member's algorithm whichever form runs it); the level shapes and
splits the cases rest on are asserted by tests/test_newton_ensemble_launch_krylov_host.py.

Splits (`tail_max_cells`): 16 -- case A has the launch levels (64), (32), case B (8,8,8), (4,4,4) with the tail (4,2,2): the
transition below launch level 1 merges some axes only (residual + `mean_children`); 64 -- one launch level in both cases,
in case B a coarse correction by the tail with two cycles.

The budgets are those of tests/test_newton_ensemble_krylov_gpu.py: K_A = 60, K_B = 40, K_B32 = 24 (case B in float32), set
from the single run `gmg.StencilGMG.solve` on the hard member of each case -- the reference, not the code under test -- by
the rule "at most K / 1.3 passes with krylov='auto', not converged at 1.3 K cycles with krylov='never'", which
`test_the_single_runs_set_the_budgets` repeats here.  Passes of the hard member, measured on an MI355X (hand-over before
cycle 2 everywhere):
                                   single run   one-workgroup form   this form, tail_max_cells 16 / 64
    case A, 1-D 64, v = 200, f64       26              29                  29 / 29
    case B, 8^3,    v = 800, f64       29              27                  27 / 27
    case A, f32 (50 eps)               16              19                  19 / 19
    case B, f32 (50 eps)               16               -                  15 / 15
"""

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
TAILS = [16, 64]
TAIL_IDS = ["tail16", "tail64"]
TOL = 1e-10
BASE_METHOD = "gmg-vcycle (variable coefficients), batched launches"

benign_members, case_arrays, CASE_A, CASE_B, CASES = (model.benign_members, model.case_arrays, model.CASE_A, model.CASE_B,
                                                           model.CASES)
K_A, K_B = CASE_A[2], CASE_B[2]
K_B32 = 24
F32_FACTOR = 4.0  # (twice the largest measured ratio, not below the 4 of the one-workgroup form's test: see the test)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def tolerance(dtype):
    """The driver's: at least 50 eps of the working precision."""
    return max(TOL, 50 * float(torch.finfo(dtype).eps))


def budget_of(case, dtype):
    return K_B32 if case[0] == "B" and dtype == F32 else case[2]


def krylov_class():
    from odil_amd import gmg

    return gmg.EnsembleLaunchKrylovGMG


def base_class():
    from odil_amd import gmg

    return gmg.EnsembleLaunchGMG


def launch(cls, coeffs, b, dtype, dev, maxcycles, tail, start=2, prepare=None, fill=0.0):
    """(x, history, outcome, [status], solver) of one solve of members `coeffs` / `b` (NumPy float64) in `dtype`."""
    ct = torch.tensor(coeffs, dtype=dtype, device=dev)
    bt = torch.tensor(b, dtype=dtype, device=dev)
    ens = cls.from_coeffs(ct, tail_max_cells=tail)
    if prepare is not None:
        prepare(ens)
    x = torch.full_like(bt, fill)
    ens.solve(bt, x, tol=tolerance(dtype), maxcycles=maxcycles, start=start)
    torch.cuda.synchronize()
    return x, ens.history.copy(), ens.outcome.copy(), [ens.status(m) for m in range(ct.shape[0])], ens


def same_bits(one, m, other, i):
    """Member m of the solve `one` = member i of the solve `other`: x, history and outcome, bit for bit."""
    return (torch.equal(one[0][m], other[0][i]) and np.array_equal(one[1][m], other[1][i])
            and np.array_equal(one[2][m], other[2][i]))


# ------------------------------------------------------------------------------------- 1: benign members, nothing changes
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", [(64,), (16, 16), (8, 8, 8)], ids=["64", "16x16", "8^3"])
def test_benign_members_keep_every_bit(dev, shape, dtype):
    coeffs = benign_members(shape, 3)
    rng = np.random.default_rng(11)
    b = np.stack([sg.apply(list(c), rng.standard_normal(shape)) for c in coeffs])  # (a rough solution: model.case_arrays)
    for tail in TAILS:
        for start in (2, 0):
            xn, hn, on, sn, base = launch(base_class(), coeffs, b, dtype, dev, 60, tail, start)
            xa, ha, oa, sa, ens = launch(krylov_class(), coeffs, b, dtype, dev, 60, tail, start)
            assert ens.nlaunch == base.nlaunch == (2 if tail == 16 else 1) and ens.shapes == base.shapes
            assert on.shape == (3, 2) and oa.shape == (3, 3) and ens.krylov == "auto" and ens.krylov_m == 6
            assert torch.equal(xa, xn), (shape, tail, start)
            assert np.array_equal(ha, hn) and np.array_equal(oa[:, :2], on) and (oa[:, 2] == -1).all()
            for m in range(3):
                assert sa[m]["handover"] is None and sa[m]["converged"]
                assert sa[m]["method"] == sn[m]["method"] == ens.method == BASE_METHOD


# ------------------------------------------------------------------------- 2: hard members are solved, honestly reported
def dense_matrix(coeffs):
    shape = coeffs[0].shape
    n = coeffs[0].size
    eye = np.eye(n).reshape((n,) + shape)
    return np.stack([sg.apply(list(coeffs), eye[j]).reshape(-1) for j in range(n)], axis=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("case", CASES, ids=["A-1d-64", "B-8^3"])
def test_hard_members_are_solved_and_reported(dev, case, tail, dtype):
    """float64: the residual formed on the host in float64 from the member's coefficient arrays as rounded to the working
    precision is at most 2 tol |b| (the kernels test the same quantity in another summation order; the rounding of A x,
    ~1e-13 relative here, is what the factor 2 is for).  float32: the error against the dense float64 solution is at most
    F32_FACTOR x that of the member's single `StencilGMG.solve(krylov="auto")` run; measured ratios (MI355X):
    0.097 (case A) and 0.84 (case B) on the hard members, 1.76 on case B's v = 200 member, which hands over too, 0.54 and
    0.89 on the benign ones -- the same at both splits to two digits.  Twice the largest, 3.5, is below the 4 of the
    one-workgroup form's test: F32_FACTOR = 4."""
    from odil_amd import gmg

    name, shape, _, members, hard, benign = case
    budget = budget_of(case, dtype)
    coeffs, b = case_arrays(case)
    nb = len(members)
    tol = tolerance(dtype)
    _, _, _, never, base = launch(base_class(), coeffs, b, dtype, dev, budget, tail)
    for m in hard:  # (the precondition on the parent's code: without it the case proves nothing)
        assert not never[m]["converged"], "the plain batched cycles bring the hard member {} in: {}".format(m, never[m])
    x, hist, out, auto, ens = launch(krylov_class(), coeffs, b, dtype, dev, budget, tail)
    assert ens.nlaunch == (2 if tail == 16 else 1)
    for m in range(nb):
        print("case", name, "tail", tail, dtype, "member", m, members[m][0], "never", never[m]["niter"], never[m]["converged"],
              "any", auto[m]["niter"], auto[m]["converged"], auto[m]["handover"], "residual",
              auto[m]["residual"] / auto[m]["bnorm"])
    for m in range(nb):
        assert auto[m]["converged"] and auto[m]["niter"] <= budget, (m, auto[m])
    for m in hard:
        assert auto[m]["handover"] is not None and auto[m]["handover"] >= 2
        assert auto[m]["method"] == BASE_METHOD + " + GCR(6)" and out[m, 2] == auto[m]["handover"]
    for m in benign:
        assert auto[m]["handover"] is None and auto[m]["method"] == BASE_METHOD and out[m, 2] == -1
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
            print("case", name, "tail", tail, "member", m, "float32 error", err, "single run", ref, status["niter"],
                  status["method"], "ratio", err / ref)
            assert status["converged"] and err <= F32_FACTOR * ref, (m, err, ref)


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
            print("budget", name, dtype, "member", m, "auto", auto["niter"], auto["method"], auto["converged"], "never",
                  never["niter"], never["converged"], never["residual"] / never["bnorm"])
            assert auto["converged"] and auto["niter"] <= budget / 1.3 and "GCR" in auto["method"]
            assert not never["converged"]


# ----------------------------------------------------------------------------------------- 3: members never communicate
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("case", CASES, ids=["A-1d-64", "B-8^3"])
def test_members_never_communicate(dev, case, tail, dtype):
    """Every member of the mixed launch -- the hard ones included -- equals the same member launched alone, and at another
    position in a launch of another size (the members reversed, the first one once more at the end): the fixed-order partial
    sums and the masks."""
    name, shape, _, members, hard, benign = case
    budget = budget_of(case, dtype)
    coeffs, b = case_arrays(case)
    nb = len(members)
    mixed = launch(krylov_class(), coeffs, b, dtype, dev, budget, tail)
    order = list(range(nb))[::-1] + [0]
    other = launch(krylov_class(), coeffs[order], b[order], dtype, dev, budget, tail)
    assert any(st["handover"] is not None for st in mixed[3])
    for i, m in enumerate(order):
        assert same_bits(mixed, m, other, i), (name, "member", m, "at", i, mixed[2][m], other[2][i])
    for m in range(nb):
        alone = launch(krylov_class(), coeffs[m:m + 1], b[m:m + 1], dtype, dev, budget, tail)
        assert same_bits(mixed, m, alone, 0), (name, "member", m, "alone", mixed[2][m], alone[2][0])
        assert mixed[3][m] == alone[3][0]


# ------------------------------------------------------------------- 3b: the pair kernel inside the GCR sequence
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("case", CASES, ids=["A-1d-64", "B-8^3"])
def test_the_gcr_sequence_through_the_pair_kernel_keeps_every_bit(dev, monkeypatch, case, tail, dtype):
    """From 2^20 cells of all members together (16 x 256^2) the cycle smooths two sweeps per pass
    (odil_stencil_var_smooth2_batch), and in the GCR sequence the last pair writes e straight into a row of the store:
    a strided [B, *shape] view, member stride 2 m cells.  With `pair_min_cells` = 0 every launch level of the cases
    pairs (their shapes are ones the pair kernel admits); x, history and outcome are those of single sweeps, hard members
    included."""
    from odil_amd import gmg, ops

    name, shape, _, members, hard, _ = case
    budget = budget_of(case, dtype)
    coeffs, b = case_arrays(case)
    assert ops.smooth2_supported(shape)
    monkeypatch.setattr(gmg.EnsembleLaunchGMG, "pair_min_cells", math.inf)
    single = launch(krylov_class(), coeffs, b, dtype, dev, budget, tail)
    assert not any(single[4].pair_eligible(lvl) for lvl in range(single[4].nlaunch))
    monkeypatch.setattr(gmg.EnsembleLaunchGMG, "pair_min_cells", 0)
    paired = launch(krylov_class(), coeffs, b, dtype, dev, budget, tail)
    assert all(paired[4].pair_eligible(lvl) for lvl in range(paired[4].nlaunch))
    for m in hard:
        assert paired[3][m]["handover"] is not None and paired[3][m]["converged"]
    for m in range(len(members)):
        assert same_bits(paired, m, single, m), (name, m, paired[2][m], single[2][m])


# --------------------------------------------------------------------------------------------- 4: the restart of GCR
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
def test_the_restart_of_gcr_is_exercised(dev, tail, dtype):
    """Case A's v = 200 member takes more passes after its hand-over than GCR keeps directions."""
    coeffs, b = case_arrays(CASE_A)
    _, _, _, auto, _ = launch(krylov_class(), coeffs, b, dtype, dev, K_A, tail)
    st = auto[1]
    print("restart", dtype, "tail", tail, "passes", st["niter"], "hand-over", st["handover"])
    assert st["converged"] and st["niter"] - st["handover"] > 6


# -------------------------------------------------------------------------- 5: a breakdown of GCR ends the member alone
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
def test_a_preconditioner_that_returns_nothing_is_a_breakdown(dev, tail, dtype):
    """A numerical input, no fault -- that of the one-workgroup form's test: sweeps that change nothing (`_set_cycle` with
    weights 0: the batched cycle's first sweep carries the norm, so the sweeps stay and do nothing) and an all-zero coarsest
    inverse.  The cycle returns its start, so the residual stays what it was -- the hand-over rule fires before cycle 2 --
    and as the preconditioner of GCR it returns e = 0, so |q|^2 = 0: stop reason 4, converged=False, the iterate (zero)
    untouched and finite.  The same operators with their real inverse and sweeps converge."""
    shape = (16, 16)
    coeffs = benign_members(shape, 2, seed=7)
    rng = np.random.default_rng(4)
    b = np.stack([sg.apply(list(c), rng.standard_normal(shape)) for c in coeffs])
    _, _, out, st, _ = launch(krylov_class(), coeffs, b, dtype, dev, 20, tail)
    assert all(s["converged"] for s in st) and (out[:, 1] == 0).all()

    def nothing(ens):
        ens._set_cycle(wpre=[0.0] * len(ens.wpre), wpost=[0.0] * len(ens.wpost), inv=torch.zeros_like(ens.inv))

    x, hist, out, st, ens = launch(krylov_class(), coeffs, b, dtype, dev, 20, tail, start=0, prepare=nothing, fill=7.0)
    assert out.tolist() == [[2, 4, 2], [2, 4, 2]]
    assert torch.equal(x, torch.zeros_like(x))
    assert (hist[:, 1] == hist[:, 0]).all() and (hist[:, 2] == hist[:, 0]).all() and (hist[:, 3] == hist[:, 0]).all()
    for status in st:
        assert not status["converged"] and not status["stagnated"] and status["handover"] == 2


# ------------------------------------------------------------------------------ 6: non-finite inputs end the member alone
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
def test_a_nan_member_ends_alone(dev, tail, dtype):
    shape = (16, 16)
    coeffs = benign_members(shape, 3, seed=7)
    rng = np.random.default_rng(3)
    b = np.stack([sg.apply(list(c), rng.standard_normal(shape)) for c in coeffs])
    bad = b.copy()
    bad[1, 5, 7] = np.nan
    with_nan = launch(krylov_class(), coeffs, bad, dtype, dev, 60, tail)
    st = with_nan[3]
    assert with_nan[2][1, 1] == 3 and not st[1]["converged"] and not st[1]["stagnated"] and st[1]["handover"] is None
    without = launch(krylov_class(), coeffs[[0, 2]], b[[0, 2]], dtype, dev, 60, tail)
    for i, m in enumerate((0, 2)):
        assert st[m]["converged"]
        assert same_bits(with_nan, m, without, i), m


# ---------------------------------------------------------------------------------------------------- 7: public API
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


def _run(odil, ensemble, spec, nb, epochs, **kw):
    args, problems, states = _members(ensemble, spec, nb, epochs)
    start = [np64(s.fields["u"].array) for s in states]
    seen = [[] for _ in range(nb)]

    def callback(member, state, epoch, pinfo):
        seen[member].append((epoch, pinfo.get("linsolver"), [float(np.array(v)) for v in pinfo["norms"]]))

    arrays, info = odil.util.optimize_newton_ensemble(args, problems, states, callback, **kw)
    return problems, states, start, seen, info


DOUBLE = [" --double 1", " --double 0"]


def linear_spec(double):
    """8^3, v_b = 800 (b + 1) / 3 = 267, 533, 800: the members semi-coarsen alike; the cycle budget of case B in that
    precision."""
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


@pytest.fixture
def small_tail(monkeypatch):
    from odil_amd import gmg

    monkeypatch.setattr(gmg.EnsembleLaunchGMG, "tail_max_cells", 64)


@pytest.mark.parametrize("double", DOUBLE, ids=DTYPE_IDS)
def test_optimize_newton_ensemble_hands_hard_members_over_across_the_launches(dev, small_tail, double):
    """The dense float64 comparison holds the float64 run only (the bound of the float64 acceptance carried through
    |M^-1|; in float32 the rounding of M d is of the order of the tolerance)."""
    from odil_amd import gmg

    odil, ensemble = _api()
    nb = 3
    LINEAR = linear_spec(double)
    problems, states, start, seen, info = _run(odil, ensemble, LINEAR, nb, 1, form="launches", krylov="any")
    assert states[0].fields["u"].array.dtype == (F64 if double.endswith("1") else F32)
    assert info.route == "stencil" and info.form == "launches" and info.handover.shape == (nb, 1)
    assert type(info.solver) is gmg.EnsembleLaunchKrylovGMG and info.solver.nlaunch == 1
    print("api handover", info.handover[:, 0], "passes", info.cycles[:, 0])
    assert info.handover[nb - 1, 0] >= 2
    for m in range(nb):
        (epoch0, none, _), (epoch1, st, _) = seen[m]
        assert none is None and st["converged"], (m, st)
        assert (st["handover"] is None) == (info.handover[m, 0] < 0)
        assert st["method"] == BASE_METHOD + ("" if st["handover"] is None else " + GCR(6)")
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
    _, _, _, seen, info = _run(odil, ensemble, LINEAR, nb, 1, form="launches", krylov="never")
    assert (info.handover == -1).all() and not seen[nb - 1][1][1]["converged"]
    assert type(info.solver) is gmg.EnsembleLaunchGMG
    # form 'auto' keeps the one-workgroup form for these members, where 'any' is 'auto'
    _, _, _, _, info = _run(odil, ensemble, LINEAR, nb, 1, form="auto", krylov="any")
    assert info.form == "workgroup" and type(info.solver) is gmg.EnsembleGMG and info.solver.krylov == "auto"


@pytest.mark.parametrize("double", DOUBLE, ids=DTYPE_IDS)
def test_any_in_the_one_workgroup_form_is_auto(dev, double):
    odil, ensemble = _api()
    nb = 3
    results = dict()
    for krylov in ("auto", "any"):
        _, states, _, seen, info = _run(odil, ensemble, linear_spec(double), nb, 1, form="workgroup", krylov=krylov)
        assert info.form == "workgroup" and info.solver.krylov == "auto"
        results[krylov] = ([s.fields["u"].array.clone() for s in states], info.cycles.copy(), info.handover.copy(),
                           [seen[m][1][1] for m in range(nb)])
    auto, any_ = results["auto"], results["any"]
    assert all(torch.equal(a, n) for a, n in zip(auto[0], any_[0]))
    assert np.array_equal(auto[1], any_[1]) and np.array_equal(auto[2], any_[2]) and auto[3] == any_[3]
    assert auto[2][nb - 1, 0] >= 2


@pytest.mark.parametrize("double", DOUBLE, ids=DTYPE_IDS)
def test_nonlinear_members_converge_step_by_step(dev, small_tail, double):
    """The norms fall from epoch to epoch down to the rounding floor of the residual evaluation in the working precision,
    as tests/test_newton_ensemble_krylov_gpu.py states it: ~8 d operations per cell on terms of size |c0| |u|, each rounded
    to eps; |c0| <= 2 d k_max N^2 + v N + 3 beta u^2 with k_max = 11, N = 8, v = 800, |u| <= 1."""
    odil, ensemble = _api()
    nb, epochs = 3, 3
    spec = linear_spec(double) + " --beta 1"
    eps = float(torch.finfo(F64 if double.endswith("1") else F32).eps)
    floor = 8 * 2 * eps * (2 * 3 * 11 * 64 + 800 * 8 + 3) * 1.0
    _, _, _, seen, info = _run(odil, ensemble, spec, nb, epochs, form="launches", krylov="any")
    assert info.route == "stencil" and info.form == "launches" and (info.handover[nb - 1] >= 2).all()
    for m in range(nb):
        assert [e for e, _, _ in seen[m]] == [0, 1, 2, 3]
        assert all(st["converged"] for _, st, _ in seen[m][1:]), (m, seen[m])
        norms = [n[0] for _, _, n in seen[m]]
        print("nonlinear member", m, "norms", norms, "handover", info.handover[m])
        assert norms[1] < norms[0]
        assert all(after < before or before <= floor for before, after in zip(norms, norms[1:])), (m, norms, floor)


# ------------------------------------------------------------------------- 8: the default split, beyond one workgroup
BIG = (256, 160)
V_LIST = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
V_RECORDED = 125.0  # (MI355X; the single run on the v = 125 member: 12 passes, hand-over to GCR)


def big_member(m, nb, velocity):
    """Member m of the sweep of examples/diffusion/ensemble.py on 256 x 160 cells (the example builds cubes only: this is
    its operator restated by tests/stencil_gmg_np.py): k = 1 + a_m 10 prod sin^2(pi x), a_m = (m + 1) / nb, and upwind
    convection - v_m du/dx_0 with v_m = velocity a_m."""
    amp = (m + 1) / nb
    kfun = lambda *xs: 1.0 + amp * 10.0 * np.prod([np.sin(np.pi * x) ** 2 for x in xs], axis=0)
    coeffs = sg.diffusion_coeffs(BIG, kfun)
    return np.stack(sg.add_upwind_convection(coeffs, velocity * amp, 0) if velocity else coeffs)


def test_the_default_split_beyond_one_workgroup(dev):
    """Three members of 256 x 160 cells at the class's tail_max_cells (one launch level of 40960 cells, 40 partial sums per
    product).  V is found by the single run, the reference: the smallest of V_LIST at which `StencilGMG.solve(krylov="auto")`
    hands the v = V member over and converges within 60 passes, while the three members still coarsen alike (`from_coeffs`
    raises otherwise).  Measured (MI355X): V = 125, the first of the list -- the single run takes 12 passes; the members
    with v = 42 and 83 stay with the plain cycles (9 and 15, the bits of `EnsembleLaunchGMG`), the v = 125 member is handed
    over before cycle 3 and takes 11 passes where the plain cycles take 21."""
    from odil_amd import gmg

    nb, tol = 3, TOL
    rng = np.random.default_rng(23)
    rough = rng.standard_normal((nb,) + BIG)
    found = None
    for velocity in V_LIST:
        coeffs = np.stack([big_member(m, nb, velocity) for m in range(nb)])
        b = np.stack([sg.apply(list(c), u) for c, u in zip(coeffs, rough)])
        ct = torch.tensor(coeffs, dtype=F64, device=dev)
        bt = torch.tensor(b, dtype=F64, device=dev)
        single = dict()
        gmg.StencilGMG(ct[nb - 1].contiguous()).solve(bt[nb - 1].contiguous(), tol=tol, maxiter=60, status=single, krylov="auto")
        try:
            ens = gmg.EnsembleLaunchKrylovGMG.from_coeffs(ct)
            alike = True
        except ValueError as refusal:
            alike = str(refusal)
        print("default split, V", velocity, "single run", single["niter"], single["method"], single["converged"], "alike", alike)
        if "GCR" in single["method"] and single["converged"] and single["niter"] <= 60 and alike is True:
            found = velocity
            break
    benign_only = found is None
    if benign_only:  # (no velocity of the list qualifies: the benign-bits half alone, on the pure-diffusion members)
        coeffs = np.stack([big_member(m, nb, 0.0) for m in range(nb)])
        b = np.stack([sg.apply(list(c), u) for c, u in zip(coeffs, rough)])
        ct, bt = torch.tensor(coeffs, dtype=F64, device=dev), torch.tensor(b, dtype=F64, device=dev)
        ens = gmg.EnsembleLaunchKrylovGMG.from_coeffs(ct)
    assert ens.nlaunch == 1 and math.prod(BIG) > gmg.EnsembleGMG.max_cells
    x = torch.zeros_like(bt)
    ens.solve(bt, x, tol=tol, maxcycles=60, start=2)
    status = [ens.status(m) for m in range(nb)]
    base = gmg.EnsembleLaunchGMG.from_coeffs(ct)
    xb = torch.zeros_like(bt)
    base.solve(bt, xb, tol=tol, maxcycles=60, start=2)
    for m in range(nb):
        print("default split, member", m, status[m]["niter"], status[m]["handover"], status[m]["converged"], "base",
              base.status(m)["niter"], base.status(m)["converged"])
    benign = [m for m in range(nb) if status[m]["handover"] is None]
    assert benign, "no member of the launch stays with the plain cycles"
    for m in benign:
        assert torch.equal(x[m], xb[m]) and np.array_equal(ens.history[m], base.history[m])
        assert np.array_equal(ens.outcome[m, :2], base.outcome[m]) and ens.outcome[m, 2] == -1
    assert found == V_RECORDED, (found, V_RECORDED)
    if benign_only:
        return
    assert status[nb - 1]["handover"] is not None and status[nb - 1]["handover"] >= 2
    for m in range(nb):
        assert status[m]["converged"] and status[m]["niter"] <= 1.3 * single["niter"], (m, status[m], single)
        res = np.linalg.norm(sg.apply(list(coeffs[m]), np64(x[m])) - b[m])
        assert res <= 2 * tol * np.linalg.norm(b[m]), (m, res)
