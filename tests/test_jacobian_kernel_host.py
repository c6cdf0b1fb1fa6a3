"""CPU check of what the generated Jacobian kernel `k_jac` computes (odil_amd/stencil_gather._jacobian_kernel): the
expressions it is emitted from (`jac_exprs`, one per entry of `jac_items`), evaluated with the NumPy DAG interpreter
(tests/dag_eval.py), labelled and collected as `TracedOperator.eval_operator_grad` does and assembled into a matrix
(tests/jacobian_ref.assemble), must be the dense float64 Jacobian torch autograd gives for the same operator run through
the oracle's `Context` (tests/jacobian_ref.dense_jacobian) -- on random NONLINEAR operators over two plain fields in one,
two and three dimensions (tests/random_ops.py, params=False), down to extents of 3 and 4 where shifts of +-2 address one
column.  The HIP kernel generated from the same expressions is held to the same reference on the GPU
(tests/test_jacobian_kernel_gpu.py), whose seeds are taken from the ones that pass here.

Bound: 1e-13 of the largest entry (values: of the largest value) -- both sides are float64 evaluations of the same formulas,
a dozen operations deep, that differ by the rounding of each; measured worst over the cases below: 5.5e-16."""

import os

import jacobian_ref as jr
import numpy as np
import pytest
from dag_eval import DagEval
from random_ops import random_case

import odil_amd as odil
from odil_amd import runtime, stencil_grad, stencil_jit
from odil_amd.stencil_codegen import _Codegen
from odil_amd.stencil_trace import TraceUnsupported

SHAPES = [(5,), (37,), (3, 5), (4, 9), (7, 13), (3, 4, 5), (5, 6, 7)]
SEEDS = [s for s in range(36) if s % 3]  # (seed % 3 == 0: an output on a window, which `k_jac` refuses -- below)
TOL = 1e-13


@pytest.fixture()
def cpu_mod():
    saved, saved_log = runtime._mod, odil.util.g_log_file
    runtime._mod = odil.ModRocm(device="cpu")
    odil.util.set_log_file(open(os.devnull, "w"))
    yield runtime._mod
    runtime._mod = saved
    odil.util.g_log_file = saved_log


def generate(problem, state):
    """The code generator with its Jacobian kernel emitted, as `TracedOperator(problem, state, jac=True)` runs it (no compiler)."""
    tr, outs, raw, names, G = stencil_jit.trace_outputs(problem, state)
    cg = _Codegen(tr, outs, raw, G, state, jac=True)
    cg.source()
    return tr, outs, cg, G


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("seed", SEEDS)
def test_jacobian_expressions_equal_the_dense_float64_jacobian(cpu_mod, seed, shape):
    problem, state, operator, rows, arrays = random_case(seed, shape)
    tr, outs, cg, G = generate(problem, state)
    assert G == tuple(shape) and len(cg.jac_exprs) == len(cg.jac_items) > len(outs)
    ev = DagEval(tr, G, dict(arrays), problem.tracers)
    # collected as stencil_jit.TracedOperator.eval_operator_grad collects the kernel's arrays
    values, grads = [None] * len(outs), [dict() for _ in outs]
    for (k, attr), e in zip(cg.jac_items, cg.jac_exprs):
        a = np.asarray(ev(e), dtype=np.float64) * np.ones(G)
        if attr is None:
            assert values[k] is None
            values[k] = a
            continue
        key, shift, loc, frozen = attr
        label = (key, tuple(int(v) for v in shift), loc)
        # the label is a read of this output that is differentiated: a live read node of its DAG, once
        reads = {tuple(n.attr) for n in stencil_grad.subdag(outs[k]) if n.op == "read"}
        assert tuple(attr) in reads and not frozen and key in ("a", "b") and loc == "c" * len(G), (k, attr)
        assert label not in grads[k], "two arrays of output {} under one label {}".format(k, label)
        grads[k][label] = a
    for k, o in enumerate(outs):  # a frozen read has no item (and the seeds do freeze reads: counted below)
        for n in stencil_grad.subdag(o):
            if n.op == "read" and n.attr[3]:
                assert (k, tuple(n.attr)) not in [(j, tuple(a) if a else a) for j, a in cg.jac_items]
    want_values = jr.values(operator, problem.domain, arrays, rows)
    want = jr.dense_jacobian(operator, problem.domain, arrays, rows)
    n = int(np.prod(G))
    for k, (v, w) in enumerate(zip(values, want_values)):
        print("value {}: {:.2e}".format(k, np.max(np.abs(v - w)) / np.max(np.abs(w))))
        assert np.max(np.abs(v - w)) <= TOL * np.max(np.abs(w)), ("value", k)
    got = jr.assemble(values, grads, ["a", "b"], G)
    jr.check_pairs(grads, want, ["a", "b"], G)
    assert got.shape == want.shape == (len(outs) * n, 2 * n)
    for k in range(len(outs)):
        rows_k = slice(k * n, (k + 1) * n)
        scale = np.max(np.abs(want[rows_k]))
        err = np.max(np.abs(got[rows_k] - want[rows_k]))
        print("jacobian of output {}: {:.2e}".format(k, err / max(scale, 1e-300)))
        assert err <= TOL * max(scale, 1e-300), ("jacobian of output", k, err / max(scale, 1e-300))
    # the matrix-free products of the helper are the products with that matrix (the GPU test relies on them at sizes
    # where the matrix is not formed)
    rng = np.random.default_rng(seed)
    v = {key: rng.standard_normal(G) for key in ("a", "b")}
    y = rng.standard_normal(len(outs) * n)
    flat = np.concatenate([v["a"].reshape(-1), v["b"].reshape(-1)])
    assert np.allclose(jr.apply(values, grads, ["a", "b"], G, v), got @ flat, rtol=0, atol=1e-12 * np.abs(got).max())
    assert np.allclose(jr.apply_transposed(values, grads, ["a", "b"], G, y), got.T @ y, rtol=0, atol=1e-12 * np.abs(got).max())
    assert np.allclose(jr.jvp(operator, problem.domain, arrays, v, rows), want @ flat, rtol=0, atol=1e-12 * np.abs(want).max())
    assert np.allclose(jr.vjp(operator, problem.domain, arrays, y, rows), want.T @ y, rtol=0, atol=1e-12 * np.abs(want).max())


def test_the_sample_is_nonlinear_and_freezes_reads(cpu_mod):
    """What makes the cases above worth running: most operators' Jacobians change with the state, and some reads are
    frozen (they must stay without an array) -- counted on the smallest two-dimensional shape."""
    nonlinear = frozen = 0
    for seed in SEEDS:
        problem, state, operator, rows, arrays = random_case(seed, (4, 9))
        J0 = jr.dense_jacobian(operator, problem.domain, arrays, rows)
        J1 = jr.dense_jacobian(operator, problem.domain, {k: a * 0.5 + 0.25 for k, a in arrays.items()}, rows)
        nonlinear += bool(np.max(np.abs(J0 - J1)) > 1e-6 * np.max(np.abs(J0)))
        tr, outs, cg, G = generate(problem, state)
        frozen += any(n.op == "read" and n.attr[3] for o in outs for n in stencil_grad.subdag(o))
    assert nonlinear >= len(SEEDS) * 3 // 4 and frozen >= 3, (nonlinear, frozen)


@pytest.mark.parametrize("shape", [(37,), (7, 13), (5, 6, 7)], ids=lambda s: "x".join(map(str, s)))
def test_windowed_outputs_are_refused_for_that_reason_only(cpu_mod, shape):
    """seed % 3 == 0 adds an output on a window of the grid: no `k_jac` (Problem.eval_operator_grad then takes the autograd
    route, tests/test_jacobian_kernel_gpu.py), and for no other reason."""
    for seed in range(0, 36, 3):
        problem, state, operator, rows, arrays = random_case(seed, shape)
        with pytest.raises(TraceUnsupported, match="not a plain residual on the whole grid"):
            generate(problem, state)
