"""The generated kernels of random programs on STAGGERED and FOUR-DIMENSIONAL grids against a float64 CPU reference
(tests/traced_cases.py, STAGGERED_CASES; the host side of the same table: tests/test_traced_staggered_host.py): reads that
pad 'c' -> 'n' or trim 'n' -> 'c', the irregular gathers behind them, node-centred grids with odd extents, outputs on two
grids (`TracedGroups`: one kernel set per grid, gradients summed), the fourth index of the prologue, of the offsets and of
the merged gather, and the multigrid transposes of `nccc` fields -- on grids where both copies of `k_fwd` run.

Every case goes through `Problem.eval_loss_grad` on the traced path and is held to `oracle.odil_generic.eval_loss_grad` in
float64 (a float32 case: on its float32-rounded inputs) in the measures of tests/test_traced_random_nd_gpu.py, with its
bounds: 1e-11 in float64, 2e-5 in float32 (the stated bounds of the generated kernels, stencil_codegen.py).  A float32
evaluation of the float32 cases on the CPU stays within 2.3e-7 of the float64 one in every measure (the host test asserts
a tenth of the bound), so neither bound leaves room for a wrong branch.  Each test prints its figures before it asserts
(DESIGN.md section 3 records the worst per dimension)."""

import numpy as np
import pytest
import torch
from test_traced_random_nd_gpu import TOL, _np64, check_adam_inside_the_gathers, check_loss_grad

import odil_amd as odil
import traced_cases as tc

pytestmark = pytest.mark.gpu

IDS = [c.id for c in tc.STAGGERED_CASES]
TWO_GRID_IDS = [c.id for c in tc.STAGGERED_CASES if len(c.output_locs) > 1]
LABEL = "traced-staggered"


@pytest.mark.parametrize("cid", IDS)
def test_traced_kernels_equal_the_float64_reference(cid, monkeypatch):
    """Loss, every term and every gradient array (all multigrid levels, `coeff`) against the reference, relative to the
    largest gradient entry and to the largest field-gradient entry; equal bits on a second call; and the values of the
    outputs (`Problem.eval_operator`), each relative to its own largest reference value, on grids of the shapes of the
    case's output locations."""
    case = tc.STAGGERED_BY_ID[cid]
    problem, state, ref = check_loss_grad(case, monkeypatch, label=LABEL)
    with tc.environment(case):
        values, names = problem.eval_operator(state)
    assert list(names) == list(ref[4]) and len(values) == len(ref[3])
    shapes = [problem.domain.get_field_shape(loc) for loc in case.output_locs]
    per = len(values) // len(shapes)  # (every group of outputs: the same plan, the same number of outputs)
    full = [tuple(v.shape) for name, v in zip(names, values) if not name.endswith("w")]
    assert full == [s for s in shapes for name in names[:per] if not name.endswith("w")], (full, shapes)
    errs = [float(np.max(np.abs(_np64(v) - r))) / float(np.max(np.abs(r))) for v, r in zip(values, ref[3])]
    print("{} {} values: {:.2e}".format(LABEL, case.id, max(errs)))
    assert all(tuple(v.shape) == r.shape for v, r in zip(values, ref[3])) and max(errs) <= TOL[case.dtype], errs


@pytest.mark.parametrize("mode", sorted(tc.RECOMPUTE_MODES))
@pytest.mark.parametrize("cid", tc.STAGGERED_RECOMPUTE_CASES)
def test_recompute_modes_equal_the_float64_reference(cid, mode, monkeypatch):
    """Two cases per dimension with every output differentiated in registers (ODIL_TRACE_RECOMPUTE=0) and with every output
    that can be re-evaluated by the gathers (ODIL_TRACE_RECOMPUTE_ALL=1): other stored adjoints, other gathers -- the
    irregular ones among them -- the same numbers."""
    check_loss_grad(tc.STAGGERED_BY_ID[cid], monkeypatch, mode, label=LABEL, **tc.RECOMPUTE_MODES[mode])


@pytest.mark.parametrize("cid", tc.STAGGERED_ADAM_CASES)
def test_adam_inside_the_gathers_equals_the_formula(cid, monkeypatch):
    """The tracer's layout, all fields at `nccc` (regular, so `traced_cases.adam_prediction` holds as it stands): plain
    fields updated by the merged 4-D gather, multigrid fields by the chain of transposes that follows it, against the
    float64 formula on the reference gradient; every level of both fields is updated, `coeff` keeps its bits."""
    case = tc.STAGGERED_BY_ID[cid]
    assert check_adam_inside_the_gathers(case, monkeypatch, label=LABEL) == 2 * case.levels


@pytest.mark.parametrize("cid", TWO_GRID_IDS)
def test_two_kernel_sets_equal_the_autograd_path_and_sum_to_the_reference(cid, monkeypatch):
    """Outputs on two grids: the sum of the two kernel sets' losses is the reference loss, each set's terms are the
    reference's terms of its outputs, and loss, terms and gradients of the traced path agree with the generic autograd
    path of the same problem on the GPU (`enable_trace` off) within the bounds of the case's type, in the same measures
    (the autograd result in the place of the reference)."""
    case = tc.STAGGERED_BY_ID[cid]
    tol = TOL[case.dtype]
    problem, state, ref = check_loss_grad(case, monkeypatch, label=LABEL)
    rloss, rterms = ref[0], ref[1]
    groups = problem._traced
    with tc.environment(case):
        loss, grads, terms, names, norms = problem.eval_loss_grad(state)
        grads = [g.clone() for g in grads]
        parts = [part.eval_loss_grad(state) for part in groups.parts]
        torch.cuda.synchronize()
        # the same problem on the generic path: what the traced one replaces
        plain, pstate, _, _ = tc.build(case)
        monkeypatch.setattr(odil.runtime, "enable_trace", False)
        ploss, pgrads, pterms, pnames, _ = plain.eval_loss_grad(pstate)
    assert plain._traced is None and plain._fused is None and list(pnames) == list(names)
    total = sum(float(p[0]) for p in parts)
    e_sum = abs(total - rloss) / abs(rloss)
    e_parts = max(abs(float(t) - rterms[k]) / abs(rterms[k])
                  for positions, p in zip(groups.groups, parts) for k, t in zip(positions, p[2]))
    assert sorted(k for positions in groups.groups for k in positions) == list(range(len(rterms)))
    auto = (float(ploss), tuple(float(t) for t in pterms), tuple(_np64(g) for g in pgrads))
    figures, per_array = tc.measures(loss, terms, grads, auto)
    print("{} {} two grids: sum of the sets' losses {:.2e}, their terms {:.2e}; against autograd: loss {:.2e} terms {:.2e} "
          "gradients {:.2e} field gradients {:.2e}".format(LABEL, case.id, e_sum, e_parts, *figures))
    assert e_sum <= tol and e_parts <= tol, (e_sum, e_parts)
    assert max(figures) <= tol, (figures, per_array)
