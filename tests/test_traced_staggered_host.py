"""CPU side of the staggered and four-dimensional random programs (tests/traced_cases.py, STAGGERED_CASES): fields that
do not live on the grid of the outputs, node-centred grids, outputs on two grids and the (t, x, y, z) layout of the tracer
problem.  The coverage the table promises, as conditions; the fold plans of every kernel set evaluated point by point; the
generated sources built with the project's own flags; the gradient expressions of the cases whose reads are all regular
against the float64 reference; and the room the float32 bound of the GPU test (tests/test_traced_staggered_gpu.py) leaves
above a float32 evaluation of the same programs on the CPU."""

import os

import numpy as np
import pytest
from test_stencil_grad_host import cpu_mod, symbolic_gradients  # noqa: F401  (cpu_mod: a fixture)
from test_traced_random_nd_host import check_folded_predicates

import traced_cases as tc
from odil_amd import stencil_jit
from oracle import odil_np as onp

IDS = [c.id for c in tc.STAGGERED_CASES]
F32_IDS = [c.id for c in tc.STAGGERED_CASES if c.dtype == np.float32]
REGULAR_IDS = [c.id for c in tc.STAGGERED_CASES if not c.converts]
F32_BOUND = 2e-5  # the float32 bound of the GPU test (the stated bound of the float kernels, stencil_codegen.py)
_CENSUS = dict()


def census_of(case):
    """(problem, state, operator, [(cg, source, kernels) per kernel set]) of a case under its environment, traced once."""
    if case.id not in _CENSUS:
        with tc.environment(case):
            problem, state, operator, rows = tc.build(case, device="cpu")
            groups = tc.census_groups(problem, state)
        _CENSUS[case.id] = (problem, state, operator, groups)
    return _CENSUS[case.id]


def test_the_table_reaches_every_path(cpu_mod):
    """Conditions on the committed table (no measurement: a case that does not meet them is replaced in traced_cases.py)."""
    names = ["c->n read", "n->c read", "irregular gather", "vw1", "vw4", "window", "rows", "multigrid with a node axis",
             "four dimensions", "two grids", "merged 4-D gather", "remapped"]
    count, f32, dims = dict.fromkeys(names, 0), 0, set()
    for case in tc.STAGGERED_CASES:
        problem, state, operator, groups = census_of(case)
        assert len(groups) == len(set(problem.domain.get_field_shape(loc) for loc in case.output_locs)), case.id
        fwds = [kernels[0] for _, _, kernels in groups]
        assert all(f["kernel"] == "k_fwd" and f["reverse"] for f in fwds)
        # both copies of `k_fwd` run: on every single-grid case, and in at least one kernel set of a two-grid case
        assert any(tc.both_copies(f) for f in fwds), (case.id, [(f["interior"], f["waves"]) for f in fwds])
        conv = [tc.conversions(cg, state) for cg, _, _ in groups]
        assert any(c[0] or c[1] for c in conv) == case.converts, case.id
        assert set(operator.dropped) <= {"roll", "rows", "window"} and (not operator.dropped or case.converts)
        count["c->n read"] += any(c[0] for c in conv)
        count["n->c read"] += any(c[1] for c in conv)
        count["irregular gather"] += any(c[2] for c in conv)
        count["vw1"] += any(f["vw"] == 1 for f in fwds)
        count["vw4"] += any(f["vw"] == 4 for f in fwds)
        count["window"] += case.seed % 3 == 0 and "window" not in operator.dropped
        count["rows"] += "rows" in operator.kinds
        count["multigrid with a node axis"] += case.multigrid and any("n" in loc for loc in case.field_locs)
        count["four dimensions"] += case.ndim == 4
        count["two grids"] += len(groups) == 2
        count["merged 4-D gather"] += case.ndim == 4 and any("k_gat_all" in source for _, source, _ in groups)
        count["remapped"] += any(f["remapped"] for f in fwds)
        assert any(f["remapped"] for f in fwds) == bool(case.env)
        dims.add(case.ndim)
        f32 += case.dtype == np.float32
    assert all(count[k] >= 3 for k in names[:9]), count
    assert all(count[k] >= 2 for k in names[9:]), count
    assert dims == {2, 3, 4} and len(tc.STAGGERED_CASES) <= 3 * f32 + 6 and 2 * f32 <= len(tc.STAGGERED_CASES)  # (about a third)
    assert sorted(tc.STAGGERED_BY_ID[c].ndim for c in tc.STAGGERED_RECOMPUTE_CASES) == [2, 2, 3, 3, 4, 4]
    # Adam inside the gathers: the tracer's layout, plain and multigrid, every field regular and updated by its gather; the
    # gather that applies the update (the merged one) runs both of its copies in one of the two
    adam = [tc.STAGGERED_BY_ID[c] for c in tc.STAGGERED_ADAM_CASES]
    assert [c.multigrid for c in adam] == [False, True] and all(c.field_locs == ("nccc", "nccc") and not c.converts for c in adam)
    sets = [census_of(case)[3][0] for case in adam]
    assert all(tc.adam_prediction(case, cg)[0] == 2 * case.levels for case, (cg, _, _) in zip(adam, sets))
    assert any(tc.both_copies(kernels[-1]) for _, _, kernels in sets)


@pytest.mark.parametrize("cid", IDS)
def test_folded_predicates_hold_away_from_the_exceptional_indices(cpu_mod, cid):
    """Per kernel set of the case: the fold constants and the folded window tests hold at every point whose indices are
    all unexceptional (the check of tests/test_traced_random_nd_host.py, on node grids and with a fourth index)."""
    problem, state, operator, groups = census_of(tc.STAGGERED_BY_ID[cid])
    checked = [check_folded_predicates(problem, cg, kernels) for cg, _, kernels in groups]
    assert any(checked), checked


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="no hipcc")
@pytest.mark.parametrize("cid", IDS)
def test_the_generated_sources_build(cpu_mod, cid):
    """`stencil_jit.trace` on CPU tensors: the case is expressed as generated kernels (one set, or one per output grid) and
    every library compiles for gfx950 with the project's flags and exports its launchers."""
    case = tc.STAGGERED_BY_ID[cid]
    with tc.environment(case):
        problem, state, operator, rows = tc.build(case, device="cpu")
        traced = stencil_jit.trace(problem, state)
    if len(case.output_locs) > 1:
        assert isinstance(traced, stencil_jit.TracedGroups) and len(traced.parts) == len(case.output_locs)
        parts = traced.parts
        assert [tuple(p.cg.G) for p in parts] == [problem.domain.get_field_shape(loc) for loc in case.output_locs]
    else:
        assert isinstance(traced, stencil_jit.TracedOperator)
        parts = [traced]
    for part in parts:
        assert os.path.exists(part.lib_path) and hasattr(part.lib, "jit_fwd")
        assert hasattr(part.lib, "jit_gather") == bool(part.cg.gathers)
    if case.converts:  # the irregular gathers are the ones generated
        assert any("k_gat_" in p.source and tc.conversions(p.cg, state)[2] for p in parts)


@pytest.mark.parametrize("cid", REGULAR_IDS)
def test_gradient_expressions_equal_the_float64_reference(cpu_mod, cid):
    """The cases all of whose reads are regular (the fields live on the output grid: the `nccc` 4-D ones): the symbolic
    gradient of "a" and "b", pulled back through the multigrid synthesis, within 1e-11 of the largest entry of the
    reference's field gradients (the bound of tests/test_traced_random_nd_host.py).  tests/dag_eval.py does not model
    converted reads, so the converting cases are held to the reference on the GPU only."""
    case = tc.STAGGERED_BY_ID[cid]
    with tc.environment(case):
        problem, state, operator, rows = tc.build(case, device="cpu", dtype=np.float64)
        loss, terms, grads, values, names = tc.reference(case, problem, state, rows)
        got, cg = symbolic_gradients(problem, state, tc.regular_arrays(problem, state))
    per = case.levels
    scale = max(np.max(np.abs(g)) for g in grads[:2 * per])
    assert np.isfinite(loss) and scale > 0 and tuple(cg.G) == problem.domain.get_field_shape(case.output_locs[0])
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


@pytest.mark.parametrize("cid", F32_IDS)
def test_the_float32_bound_leaves_no_room_for_a_wrong_branch(cpu_mod, cid):
    """Every float32 case evaluated on the CPU in float32 and in float64 on the same float32-rounded inputs
    (oracle.odil_generic): the four measures of the GPU test stay below ONE TENTH of its float32 bound, so a kernel that
    passes is within rounding of the reference and not merely within a generous bound.  Measured over this table: at most
    2.3e-7 in any measure (the 1-D .. 3-D table: 4e-7)."""
    case = tc.STAGGERED_BY_ID[cid]
    with tc.environment(case):
        problem, state, operator, rows = tc.build(case, device="cpu")
        ref = tc.reference(case, problem, state, rows)
        loss, terms, grads, values, names = tc.cpu_evaluation(case, problem, state, rows, np.float32)
    figures, _ = tc.measures(loss, terms, grads, ref)
    e_values = max(float(np.max(np.abs(v - r))) / float(np.max(np.abs(r))) for v, r in zip(values, ref[3]))
    print("traced-staggered {} float32 on the CPU: loss {:.2e} terms {:.2e} gradients {:.2e} field gradients {:.2e} values {:.2e}".format(
        case.id, *figures, e_values))
    assert max(figures) <= F32_BOUND / 10 and e_values <= F32_BOUND / 10, (figures, e_values)
