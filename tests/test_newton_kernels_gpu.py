"""The Newton stencil kernels of csrc/newton.hip (odil_stencil_apply, odil_csr_assemble, odil_stencil_march), each in
f64 and f32, called through `ops` on seeded random operators and compared with a float64 scipy.sparse restatement of
the rule include/odil_hip.h states -- row r of M holds coeffs[s][r] on column roll(arange, -shift_s)[r] -- built here
by index arithmetic, never from the kernels' own output:

  * apply     M x and M^T x against A @ x and A.T @ x (tolerance relative to |A| @ |x|) and <M x, y> = <x, M^T y>, in
              1-4 dimensions with extents 1, 2, odd and prime, shifts from [-n - 2, n + 2] per axis (0, +-(n - 1), +-n
              and a repeated shift always among them), 1, 7 and 32 shifts, above 2^20 cells, an axis longer than 65536,
              and one of more than 2^28 cells, where the grid-stride loop takes a second trip
  * assemble  indptr / indices / data equal to the restatement (shift order within a row), col_offset 0, small, > 2^31
  * march     operators triangular along one axis (either direction, any axis of 1-4 dimensions, a plane wider than the
              capped grid) against spsolve of the same matrix; the output buffer starts as NaN; recognise_marching
              accepts such operators and march_solve agrees, and it refuses when one edge coefficient is nonzero
  * refusals  malformed shift counts, diagonal slots, axes and shift directions raise before any launch"""

import math
import types

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-14, torch.float32: 2e-6}  # relative to |A| @ |x|, as tests/test_block_mg_gpu.py
TOL_MARCH = {torch.float64: 1e-12, torch.float32: 1e-5}  # relative to max |x| of the float64 solve
NP = {torch.float64: np.float64, torch.float32: np.float32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def columns(shape, shifts):
    """[size, nshift] int64: the column of every row and shift -- coordinates + shift, reduced mod the extent."""
    idx = np.indices(shape, dtype=np.int64).reshape(len(shape), -1)
    cols = np.empty((idx.shape[1], len(shifts)), dtype=np.int64)
    for k, s in enumerate(shifts):
        c = np.zeros(idx.shape[1], dtype=np.int64)
        for d, n in enumerate(shape):
            c = c * n + (idx[d] + s[d]) % n
        cols[:, k] = c
    return cols


def restate(coeffs, shape, shifts, col_offset=0):
    """(indptr, indices, data) of M in the kernel's row layout: row r holds its shifts in the order given."""
    size, nshift = math.prod(shape), len(shifts)
    data = np.asarray(coeffs, dtype=np.float64).reshape(nshift, size).T.reshape(-1)
    indices = columns(shape, shifts).reshape(-1) + col_offset
    return np.arange(size + 1, dtype=np.int64) * nshift, indices, data


def matrix(coeffs, shape, shifts, absolute=False):
    """A as scipy.sparse (repeated columns add), or |A| entry by entry (absolute: before the repeats are summed).
    The data are a copy: scipy sums repeated entries in place, and restate's data can be a view of `coeffs`."""
    size = math.prod(shape)
    indptr, indices, data = restate(coeffs, shape, shifts)
    if indptr[-1] < (1 << 31):  # (SuperLU takes 32-bit indices)
        indptr, indices = indptr.astype(np.int32), indices.astype(np.int32)
    data = np.abs(data) if absolute else data.copy()
    return sp.csr_array((data, indices, indptr), shape=(size, size))


def random_shifts(rng, shape, nshift):
    """nshift shifts from [-n - 2, n + 2] per axis, the edge values 0, +-(n - 1), +-n among them and the last shift
    a repeat of an earlier one."""
    special = lambda n: [0, n - 1, -(n - 1), n, -n]
    shifts = []
    for k in range(nshift):
        if k + 1 == nshift and nshift > 1:
            shifts.append(shifts[int(rng.integers(0, k))])
        elif k < 5:
            shifts.append(tuple(special(n)[(k + d) % 5] for d, n in enumerate(shape)))
        else:
            shifts.append(tuple(int(rng.integers(-n - 2, n + 3)) for n in shape))
    return shifts


def host(t):
    return t.double().cpu().numpy().reshape(-1)


def rounded(a, dtype):
    return np.asarray(a, dtype=NP[dtype]).astype(np.float64)


APPLY_CASES = [  # (shape, nshift)
    ((1,), 1), ((2,), 7), ((7,), 7), ((13,), 32),
    ((1, 5), 7), ((2, 3), 32), ((11, 1), 7), ((17, 13), 32), ((1, 1), 7),
    ((3, 1, 5), 7), ((5, 7, 3), 32), ((2, 2, 2), 1),
    ((2, 3, 1, 5), 7), ((3, 5, 2, 7), 32), ((1, 3, 1, 2), 1),
    ((64, 129, 131), 7),  # > 2^20 cells
    ((3, 65543), 7),  # one axis longer than 65536
    ((65599,), 32),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", range(len(APPLY_CASES)))
def test_stencil_apply_and_transpose_vs_float64(dev, dtype, case):
    from odil_amd import ops

    shape, nshift = APPLY_CASES[case]
    rng = np.random.default_rng(100 + case)
    shifts = random_shifts(rng, shape, nshift)
    c = rounded(rng.standard_normal((nshift,) + shape), dtype)
    x, yv = rounded(rng.standard_normal(shape), dtype), rounded(rng.standard_normal(shape), dtype)
    A, absA = matrix(c, shape, shifts), matrix(c, shape, shifts, absolute=True)
    tc, tx, ty = (torch.tensor(v, dtype=dtype, device=dev) for v in (c, x, yv))
    mx = host(ops.stencil_apply(tc, shifts, tx))
    mty = host(ops.stencil_apply(tc, shifts, ty, transpose=True))
    for got, want, scale in ((mx, A @ x.ravel(), absA @ np.abs(x.ravel())),
                             (mty, A.T @ yv.ravel(), absA.T @ np.abs(yv.ravel()))):
        assert np.all(np.isfinite(got))
        err = np.abs(got - want)
        assert np.all(err <= TOL[dtype] * np.maximum(scale, 1e-300)), (float(np.max(err / scale)), shifts)
    # adjoint identity of the two kernels
    lhs, rhs = float(mx @ yv.ravel()), float(x.ravel() @ mty)
    bound = 4 * TOL[dtype] * float(np.abs(yv.ravel()) @ (absA @ np.abs(x.ravel())))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def test_stencil_apply_grid_stride_wraps(dev):
    """More than 2^28 cells (grid_flat caps the grid at 2^20 workgroups of 256): the last cells are the second trip of
    the grid-stride loop.  One shift: y = c x[r + s] is one rounding, so the rolled product in the same precision is
    exact."""
    from odil_amd import ops

    shape = (16385, 16387)
    assert math.prod(shape) > (1 << 28)
    gen = torch.Generator(device=dev).manual_seed(7)
    c = torch.randn((1,) + shape, generator=gen, device=dev, dtype=torch.float32)
    x = torch.randn(shape, generator=gen, device=dev, dtype=torch.float32)
    shift = (-16386, 3)  # wraps on axis 0, ordinary on axis 1
    y = ops.stencil_apply(c, [shift], x)
    assert torch.equal(y, c[0] * torch.roll(x, shifts=tuple(-s for s in shift), dims=(0, 1)))
    del y
    yt = ops.stencil_apply(c, [shift], x, transpose=True)
    assert torch.equal(yt, torch.roll(c[0] * x, shifts=shift, dims=(0, 1)))


ASSEMBLE_CASES = [((1,), 1), ((7,), 7), ((2, 3), 32), ((5, 1, 4), 7), ((2, 3, 1, 5), 7), ((3, 65543), 7),
                  ((64, 129, 131), 7)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("col_offset", [0, 5, (3 << 31) + 7])
@pytest.mark.parametrize("case", range(len(ASSEMBLE_CASES)))
def test_csr_assemble_equals_the_restatement(dev, dtype, col_offset, case):
    from odil_amd import ops

    shape, nshift = ASSEMBLE_CASES[case]
    rng = np.random.default_rng(200 + case)
    shifts = random_shifts(rng, shape, nshift)
    c = rng.standard_normal((nshift,) + shape).astype(NP[dtype])
    indptr, indices, data = ops.csr_assemble(torch.tensor(c, device=dev), shifts, shape, col_offset=col_offset)
    want_ptr, want_idx, want_data = restate(c, shape, shifts, col_offset)
    assert np.array_equal(indptr.cpu().numpy(), want_ptr)
    assert np.array_equal(indices.cpu().numpy(), want_idx)
    got = data.cpu().numpy()
    assert got.dtype == NP[dtype] and np.array_equal(got, want_data.astype(NP[dtype]))


def triangular_operator(rng, shape, axis, direction, nshift, dtype):
    """(coeffs, shifts, diag): M triangular along `axis` -- every off-diagonal shift points 1 to 3 levels back
    against `direction`, transverse components wrap -- with the coefficients zero on the rows whose neighbour would
    lie across the end of the axis (what recognise_marching requires), the diagonal 1 + U(0, 1) with a random sign
    and sum |off| <= |diag| / 2 on every row.  The diagonal sits in a random slot; one off-diagonal shift repeats."""
    n = shape[axis]
    kmax = min(3, n - 1)
    off = []
    for k in range(nshift - 1):
        if k == 0:
            s = [0] * len(shape)
            s[axis] = -direction
        elif k + 1 == nshift - 1 and k > 1:
            s = list(off[int(rng.integers(0, k))])
        else:
            s = [int(rng.integers(-m - 2, m + 3)) for m in shape]
            s[axis] = -direction * int(rng.integers(1, kmax + 1))
        off.append(tuple(s))
    diag = int(rng.integers(0, nshift))
    shifts = off[:diag] + [(0,) * len(shape)] + off[diag:]
    d = (1.0 + rng.random(shape)) * rng.choice([-1.0, 1.0], size=shape)
    c = np.empty((nshift,) + shape)
    c[diag] = d
    if nshift > 1:
        u = rng.uniform(-1.0, 1.0, (nshift - 1,) + shape)
        u *= 0.5 * np.abs(d) / np.maximum(np.abs(u).sum(axis=0), 1e-300)
        for k, s in enumerate(s_ for j, s_ in enumerate(shifts) if j != diag):
            slot = k if k < diag else k + 1
            c[slot] = u[k]
            kk = abs(s[axis])
            edge = [slice(None)] * len(shape)
            edge[axis] = slice(0, kk) if direction > 0 else slice(n - kk, n)
            c[slot][tuple(edge)] = 0.0
    return rounded(c, dtype), shifts, diag


MARCH_CASES = [  # (shape, axis, nshift)
    ((40,), 0, 1), ((40,), 0, 3), ((9, 1), 0, 7), ((17, 13), 0, 7), ((17, 13), 1, 7),
    ((5, 6, 7), 1, 32), ((6, 5, 4), 0, 7), ((4, 3, 9), 2, 7),
    ((3, 4, 5, 6), 0, 7), ((3, 4, 5, 6), 2, 32), ((2, 1, 3, 8), 3, 7),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("case", range(len(MARCH_CASES)))
def test_stencil_march_vs_spsolve(dev, dtype, direction, case):
    from odil_amd import ops

    shape, axis, nshift = MARCH_CASES[case]
    rng = np.random.default_rng(300 + case)
    c, shifts, diag = triangular_operator(rng, shape, axis, direction, nshift, dtype)
    b = rounded(rng.standard_normal(shape), dtype)
    want = spla.spsolve(matrix(c, shape, shifts).tocsc(), b.ravel())
    tb = torch.tensor(b, dtype=dtype, device=dev)
    out = torch.full_like(tb, float("nan"))  # the solve must not read what the buffer held
    got = host(ops.stencil_march(torch.tensor(c, dtype=dtype, device=dev), shifts, diag, tb, axis, direction, out=out))
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - want)) <= TOL_MARCH[dtype] * np.max(np.abs(want)), (shifts, diag)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("direction", [1, -1])
def test_stencil_march_wide_planes(dev, dtype, direction):
    """Planes of 537600 cells, more than the capped grid of 2048 x 256 threads: every thread takes two cells of a
    level.  Marching along axis 0 makes the flat-order matrix triangular, so the reference is a triangular solve."""
    from odil_amd import ops

    shape = (4, 768, 700)
    rng = np.random.default_rng(400)
    c, shifts, diag = triangular_operator(rng, shape, 0, direction, 7, dtype)
    b = rounded(rng.standard_normal(shape), dtype)
    want = spla.spsolve_triangular(matrix(c, shape, shifts), b.ravel(), lower=direction > 0)
    tb = torch.tensor(b, dtype=dtype, device=dev)
    out = torch.full_like(tb, float("nan"))
    got = host(ops.stencil_march(torch.tensor(c, dtype=dtype, device=dev), shifts, diag, tb, 0, direction, out=out))
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - want)) <= TOL_MARCH[dtype] * np.max(np.abs(want))


def hand_linearized(coeffs, shifts, shape, dtype, dev):
    """A LinearizedOperator as Problem.linearize leaves it for one field and one output: one stencil block per shift
    (what recognise_marching reads: key_to_field, nrows, ncols, blocks)."""
    from odil_amd.core import Field

    size, loc = math.prod(shape), "c" * len(shape)
    field = Field(array=torch.zeros(shape, dtype=dtype, device=dev), loc=loc)
    blocks = [(0, size, "stencil", "u", (torch.tensor(c, dtype=dtype, device=dev).reshape(-1), tuple(s), loc, shape))
              for c, s in zip(coeffs, shifts)]
    return types.SimpleNamespace(key_to_field={"u": field}, nrows=size, ncols=size, blocks=blocks)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", [((12, 9), 0, 1), ((12, 9), 0, -1), ((5, 8, 6), 1, 1), ((3, 4, 2, 9), 3, -1)])
def test_recognise_marching_and_march_solve(dev, dtype, case):
    from odil_amd import linsolver

    shape, axis, direction = case
    rng = np.random.default_rng(500 + len(shape) + axis)
    c, shifts, diag = triangular_operator(rng, shape, axis, direction, 7, dtype)
    b = rounded(rng.standard_normal(shape), dtype)
    want = spla.spsolve(matrix(c, shape, shifts).tocsc(), b.ravel())
    # the operator as linearize hands it over: shifts not reduced, the repeated shift as two blocks
    op = hand_linearized(c, shifts, shape, dtype, dev)
    rec = linsolver.recognise_marching(op)
    assert rec is not None
    assert rec[3] == shape and rec[4] == axis and rec[5] == direction
    status = dict()
    got = host(linsolver.march_solve(rec, torch.tensor(b, dtype=dtype, device=dev).reshape(-1), status))
    assert status["method"].startswith("substitution")
    assert np.max(np.abs(got - want)) <= TOL_MARCH[dtype] * np.max(np.abs(want))
    # one coefficient across the end of the axis: no longer triangular
    k = next(j for j, s in enumerate(shifts) if j != diag and abs(s[axis]) == 1 and not any(
        v for d, v in enumerate(s) if d != axis))
    bad = c.copy()
    at = [int(rng.integers(0, m)) for m in shape]
    at[axis] = 0 if direction > 0 else shape[axis] - 1
    bad[k][tuple(at)] = 0.25
    assert linsolver.recognise_marching(hand_linearized(bad, shifts, shape, dtype, dev)) is None


def test_refusals_before_any_launch(dev):
    from odil_amd import ops
    from odil_amd._lib import OdilHipError

    shape = (6, 5)
    x = torch.zeros(shape, dtype=torch.float64, device=dev)
    c33 = torch.zeros((33,) + shape, dtype=torch.float64, device=dev)
    with pytest.raises(OdilHipError):
        ops.stencil_apply(c33[:0], [], x)
    with pytest.raises(OdilHipError):
        ops.stencil_apply(c33, [(0, 0)] * 33, x)
    with pytest.raises(OdilHipError):
        ops.csr_assemble(c33[:0], [], shape)
    with pytest.raises(OdilHipError):
        ops.csr_assemble(c33, [(0, 0)] * 33, shape)
    good = [(0, 0), (-1, 0), (-2, 3)]
    c3 = c33[:3].contiguous()
    for diag, axis, direction, shifts in [
        (-1, 0, 1, good), (3, 0, 1, good),  # diagonal slot out of range
        (1, 0, 1, good),  # slot 1 is not the zero shift
        (0, -1, 1, good), (0, 2, 1, good),  # axis out of range
        (0, 0, -1, good), (0, 0, 0, good),  # wrong direction, no direction
        (0, 0, 1, [(0, 0), (-1, 0), (0, 1)]),  # a neighbour in the same level
        (0, 0, 1, [(0, 0), (-1, 0), (-6, 0)]),  # a whole period back: the same level
        (0, 0, 1, [(0, 0)] * 33),
    ]:
        coeffs = c33 if len(shifts) == 33 else c3
        with pytest.raises(OdilHipError):
            ops.stencil_march(coeffs, shifts, diag, x, axis, direction)
    with pytest.raises(OdilHipError):
        ops.stencil_march(c33[:0], [], 0, x, 0, 1)
    torch.cuda.synchronize()
