"""The generated Jacobian kernel `k_jac` (odil_amd/stencil_gather._jacobian_kernel, launched by
stencil_jit.TracedOperator.eval_operator_grad, consumed by core.LinearizedOperator) against a dense float64 Jacobian that
knows nothing of this package's tracer: torch autograd on the CPU of the same operator run through the oracle's `Context`
(tests/jacobian_ref.py).  Every Newton route starts from this kernel; a wrong coefficient array crashes nothing.

Operators: the random straight-line programs of tests/random_ops.py on two plain fields (params=False) in one, two and three
dimensions -- most of them nonlinear in the unknowns (tests/test_jacobian_kernel_host.py counts them), with masks, rolls,
rows imposed by concatenation and frozen reads; every fourth case in float32 (kernels built with other flags and the fast
intrinsics), its reference the float64 evaluation on the same float32 state.  Extents: odd, prime, smaller than the stencil's
reach (3 and 4: shifts of +-2 address one column), rows with and without the four-wide vector path, more than one workgroup.

  * small shapes: values, every entry of the matrix the coefficient arrays stand for (jacobian_ref.assemble), the set of
    keys, and `LinearizedOperator`: the vector, matvec, rmatvec and the CSR matrix of `Problem.linearize`, entry by entry;
  * larger shapes (a dense reference would take thousands of reverse passes): J v and J^T y for random directions;
  * operators `k_jac` refuses (an output on a window): the autograd route must take over and be right.

Bounds, relative to the largest entry of the reference for that output (values: the largest value; products: the largest
entry of the reference product): float64 1e-10, the project's bound for generated kernels on random operators; float32
2e-5, the bound odil_amd/stencil_codegen.py states for its float kernels.  Measured worst on an MI355X over the 54 kernel
cases below -- values, Jacobian entries, the vector and the CSR matrix: float64 5.2e-16 (seed 2 on 7 x 13), float32 2.5e-7
(seed 28 on 5 x 36); products J v, J^T y, matvec, rmatvec: float64 7.2e-16, float32 2.4e-7."""

import os

import jacobian_ref as jr
import numpy as np
import pytest
import torch
from random_ops import random_case

import odil_amd as odil

pytestmark = pytest.mark.gpu

KEYS = ["a", "b"]
TOL = {np.float64: 1e-10, np.float32: 2e-5}
SEEDS_2D = [s for s in range(36) if s % 3]  # 24 seeds
SHAPES_2D = [(8, 8), (7, 13), (5, 36), (9, 9), (3, 5), (4, 9), (9, 4), (3, 64)]
# seeds of 1-D and 3-D programs that generate `k_jac` (tests/test_jacobian_kernel_host.py runs the same generation)
DENSE = ([(s, SHAPES_2D[i % 8], np.float32 if (i + i // 8) % 4 == 0 else np.float64) for i, s in enumerate(SEEDS_2D)]
         + [(s, [(5,), (37,), (130,)][i % 3], np.float32 if i % 4 == 1 else np.float64) for i, s in enumerate([1, 2, 4, 5, 7, 8])]
         + [(s, [(3, 4, 5), (5, 6, 7), (4, 9, 36)][i % 3], np.float32 if i % 4 == 1 else np.float64)
            for i, s in enumerate([1, 2, 4, 5, 7, 8, 10, 11])])
LARGE = [(s, shape, dt) for shape, seeds in [((33, 68), (13, 14)), ((6, 515), (16, 17)), ((130, 7), (19, 20)), ((9, 10, 66), (22, 23))]
         for s in seeds for dt in (np.float64, np.float32)]
FALLBACK = [(30, (7, 13)), (36, (4, 9)), (60, (37,)), (63, (3, 4, 5))]  # seed % 3 == 0, programs without a roll (see the test)


def case_id(case):
    return "{}-{}{}".format(case[0], "x".join(map(str, case[1])), "-f32" if len(case) > 2 and case[2] == np.float32 else "")


@pytest.fixture(scope="module", autouse=True)
def quiet():
    saved = odil.util.g_log_file
    odil.util.set_log_file(open(os.devnull, "w"))
    yield
    odil.util.g_log_file = saved


def err(got, want):
    """max |got - want| relative to the largest entry of the reference"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return float(np.max(np.abs(got.astype(np.float64).reshape(-1) - np.asarray(want).reshape(-1)))) / max(float(np.max(np.abs(want))), 1e-300)


def traced_case(seed, shape, dtype):
    problem, state, operator, rows, arrays = random_case(seed, shape, dtype, "cuda:0")
    values, grads, names = problem.eval_operator_grad(state)
    assert problem._jac_traced, "the Jacobian kernel was not generated: eval_operator_grad went through autograd"
    assert list(names) == ["f0", "f1", "f2"] and len(values) == len(grads) == 3
    return problem, state, operator, rows, arrays, values, grads


def check_values(values, want, tol, what):
    for k, (v, w) in enumerate(zip(values, want)):
        e = err(v, w)
        print("{} value {}: {:.2e}".format(what, k, e))
        assert tuple(v.shape) == w.shape and e <= tol, (what, "value", k, e)


def check_blocks(got, want, nblocks, tol, what):
    """`got` against `want` block by block (per output or per field), each relative to its block of the reference"""
    n = want.shape[0] // nblocks
    assert got.shape == want.shape
    for k in range(nblocks):
        e = err(got[k * n:(k + 1) * n], want[k * n:(k + 1) * n])
        print("{} block {}: {:.2e}".format(what, k, e))
        assert e <= tol, (what, k, e)


def directions(seed, G, dtype, count):
    """random v (key -> array) and y (the outputs' layout), representable in `dtype`"""
    rng = np.random.default_rng(1000 + seed)
    n = int(np.prod(G))
    for _ in range(count):
        v = {key: rng.standard_normal(G).astype(dtype).astype(np.float64) for key in KEYS}
        yield v, rng.standard_normal(3 * n).astype(dtype).astype(np.float64)


def device_vector(a, dtype):
    return torch.as_tensor(np.asarray(a).astype(dtype)).to("cuda:0")


@pytest.mark.parametrize("case", DENSE, ids=case_id)
def test_jacobian_kernel_equals_the_dense_float64_jacobian(case):
    seed, shape, dtype = case
    tol, G = TOL[dtype], tuple(shape)
    problem, state, operator, rows, arrays, values, grads = traced_case(seed, shape, dtype)
    want_values = jr.values(operator, problem.domain, arrays, rows)
    J = jr.dense_jacobian(operator, problem.domain, arrays, rows)
    check_values(values, want_values, tol, "k_jac")
    for grad in grads:
        for (key, shift, loc), a in grad.items():
            assert key in KEYS and loc == "c" * len(G) and len(shift) == len(G) and tuple(a.shape) == G, (key, shift, loc)
    check_blocks(jr.assemble(values, grads, KEYS, G), J, 3, tol, "k_jac jacobian")
    jr.check_pairs(grads, J, KEYS, G)
    # LinearizedOperator on what the kernel wrote
    vector, op = problem.linearize_device(state)
    assert op.shape == J.shape
    check_blocks(vector.cpu().numpy().astype(np.float64), np.concatenate([w.reshape(-1) for w in want_values]), 3, tol, "vector")
    for v, y in directions(seed, G, dtype, 2):
        flat = np.concatenate([v[key].reshape(-1) for key in KEYS])
        check_blocks(op.matvec(device_vector(flat, dtype)).cpu().numpy().astype(np.float64), J @ flat, 3, tol, "matvec")
        check_blocks(op.rmatvec(device_vector(y, dtype)).cpu().numpy().astype(np.float64), J.T @ y, 2, tol, "rmatvec")
    vector, matrix = problem.linearize(state)
    check_blocks(np.asarray(matrix.toarray(), dtype=np.float64), J, 3, tol, "to_scipy")


@pytest.mark.parametrize("case", LARGE, ids=case_id)
def test_jacobian_kernel_products_on_larger_grids(case):
    seed, shape, dtype = case
    tol, G = TOL[dtype], tuple(shape)
    problem, state, operator, rows, arrays, values, grads = traced_case(seed, shape, dtype)
    want_values = jr.values(operator, problem.domain, arrays, rows)
    check_values(values, want_values, tol, "k_jac")
    vector, op = problem.linearize_device(state)
    check_blocks(vector.cpu().numpy().astype(np.float64), np.concatenate([w.reshape(-1) for w in want_values]), 3, tol, "vector")
    for v, y in directions(seed, G, dtype, 4):
        flat = np.concatenate([v[key].reshape(-1) for key in KEYS])
        Jv, JTy = jr.jvp(operator, problem.domain, arrays, v, rows), jr.vjp(operator, problem.domain, arrays, y, rows)
        check_blocks(jr.apply(values, grads, KEYS, G, v), Jv, 3, tol, "k_jac J v")
        check_blocks(jr.apply_transposed(values, grads, KEYS, G, y), JTy, 2, tol, "k_jac J^T y")
        check_blocks(op.matvec(device_vector(flat, dtype)).cpu().numpy().astype(np.float64), Jv, 3, tol, "matvec")
        check_blocks(op.rmatvec(device_vector(y, dtype)).cpu().numpy().astype(np.float64), JTy, 2, tol, "rmatvec")


@pytest.mark.parametrize("case", FALLBACK, ids=case_id)
def test_operators_without_a_jacobian_kernel_take_the_autograd_route(case):
    """seed % 3 == 0: a fourth output on a window of the grid, which `k_jac` refuses -- `eval_operator_grad` must fall back
    to one autograd pass per output and still be right.  That route (as the reference's, core.py:1313-1361) differentiates
    the SUM of an output with respect to every read: per read the column sums of the output's Jacobian, which are its
    coefficient arrays when the output is pointwise in its reads.  So: programs without a `roll` step, whose three whole-grid
    outputs are pointwise, pass the dense comparison of the kernel cases; the window output (not pointwise: `linearize`
    refuses it) is held to the column sums of its dense block."""
    seed, shape = case
    G, n, tol = tuple(shape), int(np.prod(shape)), TOL[np.float64]
    problem, state, operator, rows, arrays = random_case(seed, shape, np.float64, "cuda:0")
    assert "roll" not in operator.kinds
    values, grads, names = problem.eval_operator_grad(state)
    assert problem._jac_traced is False
    assert list(names) == ["f0", "f1", "f2", "w"]
    want_values = jr.values(operator, problem.domain, arrays, rows)
    J = jr.dense_jacobian(operator, problem.domain, arrays, rows)
    check_values(values, want_values, tol, "autograd")
    check_blocks(jr.assemble(values[:3], grads[:3], KEYS, G), J[:3 * n], 3, tol, "autograd jacobian")
    jr.check_pairs(grads[:3], J[:3 * n], KEYS, G)
    sums = np.zeros(2 * n)
    for (key, shift, loc), a in grads[3].items():
        if a is not None:
            np.add.at(sums, KEYS.index(key) * n + jr.columns(shift, G), a.detach().cpu().numpy().astype(np.float64).reshape(-1))
    check_blocks(sums, J[3 * n:].sum(axis=0), 2, tol, "autograd window column sums")
    with pytest.raises(ValueError, match="not pointwise"):
        problem.linearize_device(state)
