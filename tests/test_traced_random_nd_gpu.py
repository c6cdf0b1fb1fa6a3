"""The generated kernels of random 1-D, 2-D and 3-D programs against a float64 CPU reference, on grids where BOTH copies of
their bodies run (tests/traced_cases.py; the host side of the same table: tests/test_traced_random_nd_host.py).

Every case goes through `Problem.eval_loss_grad` on the traced path -- `k_fwd`, the gathers, the multigrid transposes --
and is compared with `oracle.odil_generic.eval_loss_grad` in float64 (for a float32 case: on the float32-rounded inputs):
the loss and every term relative to the reference value, every gradient array (multigrid levels and `coeff` included) in
the max norm relative to the largest entry of all reference gradients -- and the fields' arrays also relative to the
largest entry among themselves, the stricter measure wherever `coeff` has the largest gradient.  Bounds: 1e-11 in float64
(the bound the gradient expressions are held to on the host) and 2e-5 in float32 (the stated bound of the float kernels,
stencil_codegen.py); a float32 CPU evaluation of the same cases differs from the float64 one by at most 4e-7 in either
measure, so neither bound leaves room for a wrong branch.  Twelve cases repeat under the two other recompute modes, six
run the Adam update inside the gathers.  Each test prints its figures before it asserts (DESIGN.md section 3 records the
worst)."""

import numpy as np
import pytest
import torch

import odil_amd as odil
import traced_cases as tc

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-11, np.float32: 2e-5}
IDS = [c.id for c in tc.CASES]


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _traced(problem, state, monkeypatch, groups=1):
    """The evaluator of the problem on its generated kernels: a `TracedOperator`, or (groups > 1: outputs on that many
    grids) a `TracedGroups` of that many kernel sets."""
    monkeypatch.setattr(odil.runtime, "enable_trace", True)
    problem.recognise(state)
    from odil_amd.stencil_jit import TracedGroups, TracedOperator

    assert isinstance(problem._traced, TracedOperator if groups == 1 else TracedGroups), "the case must run on its generated kernels"
    assert groups == 1 or len(problem._traced.parts) == groups
    return problem._traced


def check_loss_grad(case, monkeypatch, mode="chosen", label="traced-nd", **env):
    """One case on the traced path, twice (equal bits: the reductions are ordered), against the reference: the four
    measures of `traced_cases.measures` (the fields' arrays are all but the `Array`).  Returns (problem, state, reference)."""
    tol = TOL[case.dtype]
    with tc.environment(case, **env):
        problem, state, operator, rows = tc.build(case)
        ref = tc.reference(case, problem, state, rows)
        _traced(problem, state, monkeypatch, len(case.output_locs))
        loss, grads, terms, names, norms = problem.eval_loss_grad(state)
        grads = [g.clone() for g in grads]  # (views of a buffer the next call overwrites)
        loss2, grads2, terms2, _, norms2 = problem.eval_loss_grad(state)
    assert list(names) == list(ref[4])
    assert np.array_equal(loss, loss2) and all(np.array_equal(a, b) for a, b in zip(list(terms) + list(norms), list(terms2) + list(norms2)))
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    (e_loss, e_term, e_grad, e_field), per_array = tc.measures(loss, terms, grads, ref)
    print("{} {} {}: loss {:.2e} terms {:.2e} gradients {:.2e} field gradients {:.2e}".format(
        label, case.id, mode, e_loss, e_term, e_grad, e_field))
    assert e_loss <= tol and e_term <= tol, (e_loss, e_term)
    assert e_grad <= tol and e_field <= tol, per_array
    return problem, state, ref


@pytest.mark.parametrize("cid", IDS)
def test_traced_kernels_equal_the_float64_reference(cid, monkeypatch):
    case = tc.BY_ID[cid]
    problem, state, ref = check_loss_grad(case, monkeypatch)
    # the values of the outputs (`Problem.eval_operator`), each in the max norm relative to its own largest reference value
    with tc.environment(case):
        values, names = problem.eval_operator(state)
    assert list(names) == list(ref[4]) and len(values) == len(ref[3])
    errs = [float(np.max(np.abs(_np64(v) - r))) / float(np.max(np.abs(r))) for v, r in zip(values, ref[3])]
    print("traced-nd {} values: {:.2e}".format(case.id, max(errs)))
    assert all(tuple(v.shape) == r.shape for v, r in zip(values, ref[3])) and max(errs) <= TOL[case.dtype], errs


@pytest.mark.parametrize("mode", sorted(tc.RECOMPUTE_MODES))
@pytest.mark.parametrize("cid", tc.RECOMPUTE_CASES)
def test_recompute_modes_equal_the_float64_reference(cid, mode, monkeypatch):
    """ODIL_TRACE_RECOMPUTE=0 (stored read cotangents and affine cuts only) and ODIL_TRACE_RECOMPUTE_ALL=1 (every output
    that can be is re-evaluated by the gathers): other stored adjoints, other gathers, the same numbers."""
    check_loss_grad(tc.BY_ID[cid], monkeypatch, mode, **tc.RECOMPUTE_MODES[mode])


ALPHA, OMB1, OMB2, EPS = 0.5, 0.5, 0.25, 1e-7  # (large on purpose: an error of the gradient shows in x, m and v undamped)


def check_adam_inside_the_gathers(case, monkeypatch, label="traced-nd"):
    """`TracedOperator.eval_loss_grad_adam` with the update forced on small grids: from random m (of the gradient's size)
    and positive v, the arrays the gathers and the multigrid chain update equal m + (g - m) (1 - b1), v + (g^2 - v) (1 - b2),
    x - alpha m / (sqrt(v) + eps) (optimizer.py; reference optimizer.py:316-318) evaluated in float64 NumPy on the
    REFERENCE gradient, in the max norm relative to the largest entry of x, m and v respectively; the other arrays keep
    their bits, and the number of updated arrays is what the layout of the state predicts (traced_cases.adam_prediction).
    Returns that number."""
    tol = TOL[case.dtype]
    monkeypatch.setenv("ODIL_FUSE_ADAM_SMALL", "1")
    with tc.environment(case):
        problem, state, operator, rows = tc.build(case)
        rloss, rterms, rgrads, _, _ = tc.reference(case, problem, state, rows)
        tro = _traced(problem, state, monkeypatch)
        x = problem.domain.arrays_from_state(state)
        scale = max(float(np.max(np.abs(g))) for g in rgrads[:-1])  # (of the fields' gradients: `coeff` is never updated here)
        gen = torch.Generator(device="cpu").manual_seed(900 + case.seed)
        tdt = x[0].dtype
        m = [(torch.randn(tuple(a.shape), generator=gen, dtype=torch.float64) * scale).to(tdt).to(a.device) for a in x]
        v = [((torch.rand(tuple(a.shape), generator=gen, dtype=torch.float64) + 0.5) * scale**2).to(tdt).to(a.device) for a in x]
        before = [[_np64(t) for t in part] for part in (x, m, v)]
        kept = [[t.clone() for t in part] for part in (x, m, v)]
        res = tro.eval_loss_grad_adam(state, m, v, ALPHA, OMB1, OMB2, EPS)
        torch.cuda.synchronize()
    done, why = tc.adam_prediction(case, tro.cg)
    print("{} {} adam: {} leading arrays ({})".format(label, case.id, done, why))
    if done == 0:
        assert res is None, why
    else:
        assert res is not None and res[-1] == done, (res and res[-1], done, why)
        loss, grads = res[0], res[1]
        assert abs(float(loss) - rloss) <= tol * abs(rloss)
        e_grad = max(float(np.max(np.abs(_np64(g).reshape(r.shape) - r))) for g, r in zip(grads[:-1], rgrads[:-1])) / scale
        assert e_grad <= tol, e_grad
    worst = dict(x=0.0, m=0.0, v=0.0)
    for k, g in enumerate(rgrads):
        x0, m0, v0 = (before[j][k] for j in range(3))
        if k >= done:
            assert all(torch.equal(part[k], old[k]) for part, old in zip((x, m, v), kept)), ("array {} was touched".format(k), why)
            continue
        m1 = m0 + (g.reshape(m0.shape) - m0) * OMB1
        v1 = v0 + (g.reshape(v0.shape) ** 2 - v0) * OMB2
        x1 = x0 - (m1 * ALPHA) / (np.sqrt(v1) + EPS)
        for name, got, want in (("x", x[k], x1), ("m", m[k], m1), ("v", v[k], v1)):
            worst[name] = max(worst[name], float(np.max(np.abs(_np64(got) - want))) / float(np.max(np.abs(want))))
    print("{} {} adam: x {x:.2e} m {m:.2e} v {v:.2e}".format(label, case.id, **worst))
    assert max(worst.values()) <= tol, worst
    return done


@pytest.mark.parametrize("cid", tc.ADAM_CASES)
def test_adam_inside_the_gathers_equals_the_formula(cid, monkeypatch):
    """The six cases of the 1-D .. 3-D table (`check_adam_inside_the_gathers`)."""
    check_adam_inside_the_gathers(tc.BY_ID[cid], monkeypatch)
