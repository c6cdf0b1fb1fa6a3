"""CPU side of the random-program cases of tests/traced_cases.py (1-D, 2-D and 3-D grids with rows longer than a
wavefront): the gradient expressions behind the generated gathers against the float64 reference, the FOLD PLANS of the
interior copies evaluated point by point, and the coverage the table promises -- on every case both copies of `k_fwd` run,
and the folded copies of the gathers, the two vector widths, windows, imposed rows, rolls, multigrid fields, the
wave-uniform index prologue and the chunk remap are each reached by several cases.  The kernels generated from these plans
are held to the same reference on the GPU (tests/test_traced_random_nd_gpu.py)."""

import numpy as np
import pytest
from dag_eval import DagEval
from test_stencil_grad_host import cpu_mod, symbolic_gradients  # noqa: F401  (cpu_mod: a fixture)

import traced_cases as tc
from oracle import odil_np as onp

IDS = [c.id for c in tc.CASES]
_CENSUS = dict()


def census_of(case):
    """(problem, state, cg, kernels) of a case under its environment, traced once per module."""
    if case.id not in _CENSUS:
        with tc.environment(case):
            problem, state, operator, rows = tc.build(case, device="cpu")
            cg, source, kernels = tc.census(problem, state)
        _CENSUS[case.id] = (problem, state, operator, cg, kernels)
    return _CENSUS[case.id]


@pytest.mark.parametrize("cid", IDS)
def test_gradient_expressions_equal_the_float64_reference(cpu_mod, cid):
    """The symbolic gradient of "a" and "b" (pulled back through the multigrid synthesis where the fields have levels)
    within 1e-11 of the largest entry of the reference's field gradients -- the bound of the 2-D 8 x 8 check of the same
    expressions (test_stencil_grad_host.py).  A float32 case is checked as the float64 problem on its float32-rounded
    numbers: that is what its reference evaluates, and the expressions do not depend on the element type."""
    case = tc.BY_ID[cid]
    with tc.environment(case):
        problem, state, operator, rows = tc.build(case, device="cpu", dtype=np.float64)
        loss, terms, grads, values, names = tc.reference(case, problem, state, rows)
        got, cg = symbolic_gradients(problem, state, tc.regular_arrays(problem, state))
    per = 2 if case.multigrid else 1
    scale = max(np.max(np.abs(g)) for g in grads[:2 * per])
    assert np.isfinite(loss) and scale > 0
    for k, key in enumerate(("a", "b")):
        want = grads[k * per:(k + 1) * per]
        if key not in got:
            assert all(np.max(np.abs(w)) == 0 for w in want)
            continue
        g = [got[key]]
        if case.multigrid:
            field = state.fields[key]
            g = onp.multigrid_to_regular_adj(got[key], [w.shape for w in want], field.loc, field.factors or problem.domain.mg_factors,
                                             problem.domain.mg_axes)
        for level, (a, b) in enumerate(zip(g, want)):
            assert np.max(np.abs(a - b)) <= 1e-11 * scale, (key, level, np.max(np.abs(a - b)) / scale, cg.out_mode)


def check_folded_predicates(problem, cg, kernels):
    """Every kernel of one kernel set with a fold plan: each folded predicate has its fold constant, and each folded window
    test holds, at every grid point none of whose indices is exceptional.  Returns the number of predicates checked."""
    G, checked = cg.G, 0
    ev = DagEval(cg.tr, G, dict(), problem.tracers)  # (index predicates read no array)
    for kernel in kernels:
        if kernel["plan"] is None:
            continue
        fold, exc, inbox = kernel["plan"]
        away = np.ones(G, dtype=bool)
        for d, values in exc.items():
            assert kernel["vw"] == 1 or d != len(G) - 1, "a four-point kernel folds nothing along the last axis"
            keep = ~np.isin(np.arange(G[d]), values)
            away &= keep.reshape([-1 if e == d else 1 for e in range(len(G))])
        assert away.any()
        for idx, const in fold.items():
            value = np.broadcast_to(np.asarray(ev(cg.tr.nodes[idx]), dtype=bool), G)
            assert np.all(value[away] == const), (kernel["kernel"], cg.tr.nodes[idx].op, const)
            checked += 1
        for k, d in inbox:
            index = np.broadcast_to(np.arange(G[d]).reshape([-1 if e == d else 1 for e in range(len(G))]), G)
            assert np.all(index[away] < cg.out_lens[k][d]), (kernel["kernel"], k, d)
            checked += 1
    return checked


@pytest.mark.parametrize("cid", IDS)
def test_folded_predicates_hold_away_from_the_exceptional_indices(cpu_mod, cid):
    """Every kernel with a fold plan: each folded predicate has its fold constant, and each folded window test holds, at
    every grid point none of whose indices is exceptional -- the points of the wavefronts that take the interior copy."""
    problem, state, operator, cg, kernels = census_of(tc.BY_ID[cid])
    assert check_folded_predicates(problem, cg, kernels)


@pytest.mark.parametrize("cid", IDS)
def test_both_copies_of_the_forward_kernel_run(cpu_mod, cid):
    """The reason the case is in the table: `k_fwd` has wavefronts that take the interior copy and wavefronts that do not."""
    problem, state, operator, cg, kernels = census_of(tc.BY_ID[cid])
    fwd = kernels[0]
    assert fwd["kernel"] == "k_fwd" and fwd["reverse"] and fwd["plan"] is not None
    assert 0 < fwd["interior"] < fwd["waves"], (fwd["interior"], fwd["waves"])


def test_the_table_reaches_every_path(cpu_mod):
    """Conditions on the committed table (no measurement: a case that does not meet them is replaced in traced_cases.py)."""
    count = dict.fromkeys(["gather", "vw1 last axis", "vw4", "window", "rows", "roll", "multigrid", "uniform", "remapped"], 0)
    dims, f32 = set(), 0
    for case in tc.CASES:
        problem, state, operator, cg, kernels = census_of(case)
        fwd, last = kernels[0], case.ndim - 1
        assert tc.both_copies(fwd)
        fold, exc, inbox = fwd["plan"]
        memo = dict()
        folded_last = any(cg._index_values(cg.tr.nodes[i], memo)[0] == last for i in fold)
        count["gather"] += any(tc.both_copies(k) for k in kernels[1:])
        count["vw1 last axis"] += fwd["vw"] == 1 and folded_last
        count["vw4"] += fwd["vw"] == 4
        count["window"] += case.seed % 3 == 0 and bool(inbox)
        count["rows"] += "rows" in operator.kinds
        count["roll"] += "roll" in operator.kinds
        count["multigrid"] += case.multigrid
        count["uniform"] += fwd["uniform"]
        count["remapped"] += fwd["remapped"]
        assert fwd["remapped"] == bool(case.env) and fwd["uniform"] == (case.ndim >= 2 and case.shape[-1] % 256 == 0)
        dims.add(case.ndim)
        f32 += case.dtype == np.float32
    assert count["gather"] >= 6, count
    assert all(n >= 3 for n in count.values()), count
    assert dims == {1, 2, 3} and 3 * f32 >= len(tc.CASES) - 3 and 4 * count["multigrid"] >= len(tc.CASES)
    assert min(c.seed for c in tc.CASES) >= 56  # (0 .. 55: the programs of tests/test_workloads_gpu.py)
    for cid in tc.RECOMPUTE_CASES:  # the cases that also run in the two other recompute modes: a gather with both copies
        assert any(tc.both_copies(k) for k in census_of(tc.BY_ID[cid])[4][1:]), cid
    assert sorted(tc.BY_ID[c].ndim for c in tc.RECOMPUTE_CASES) == [1] * 4 + [2] * 4 + [3] * 4
    assert sorted(tc.BY_ID[c].ndim for c in tc.ADAM_CASES) == [1, 1, 2, 2, 3, 3]
    # Adam inside the gathers: cases that fuse both fields, a case that fuses nothing, and the gather that applies the
    # update (the merged one) runs both of its copies in at least one case per dimension
    done = {cid: tc.adam_prediction(tc.BY_ID[cid], census_of(tc.BY_ID[cid])[3])[0] for cid in tc.ADAM_CASES}
    assert 0 in done.values() and 2 in done.values() and 4 in done.values(), done
    for nd in (1, 2, 3):
        assert any(tc.both_copies(census_of(tc.BY_ID[cid])[4][-1]) for cid in tc.ADAM_CASES if tc.BY_ID[cid].ndim == nd and done[cid])
