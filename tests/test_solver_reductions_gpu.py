"""The reductions the solvers read (odil_dots, _dots3, _lbfgs_probe, _lincomb, _mean_reduce, _max_abs_diff,
_max_abs_rows) and the two conversions of the mixed-precision refinement (odil_narrow_scale, _widen_axpy), each
called through `ops` and compared with NumPy in float64:

  * sizes     1, 255 .. 257, 2047, 2049 (block size, one block's work), 2^21 - 1 .. 2^21 + 1 (where the partial-sum grid
              caps and chunks of ceil(n / grid) begin) and 2^25 + 3 (every block loops); integer-valued inputs
              (|v| <= 8: every float64 sum is exact) must give the integer result exactly, random normal inputs agree
              to the tolerances of test_hip_kernels.test_vector_ops (float64) or to 1 ulp of float32(reference)
  * dots3     both sides of every condition of the path that reads the right-hand vectors once (nvec <= 128,
              n a multiple of the vector width, n >= 256 * 64), strided and odd-strided rows
  * lincomb   bit for bit against the same expression in the same order; beta 0 (y not read), 1 and other values;
              nvec 0, 1 and 100; lda != n
  * max       max_abs_diff / max_abs_rows exact, 1 and 64 rows, n above 2^22 where the grid caps
  * convert   narrow_scale / widen_axpy bit for bit for msq NULL, > 0, = 0 and < 0, and the round trip to 2^-24
  * non-finite  a NaN or an Inf at index 0, n - 1 and either side of a chunk boundary gives what IEEE arithmetic
              gives; the maxima (max |g| of lbfgs_probe included) carry a NaN and report +Inf for an infinite entry
  * L-BFGS-B  a NaN in the first gradient must not be reported as convergence"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK, PER_BLOCK, DOT_PARTIALS, GRID_CAP = 256, 256 * 8, 1024, 2048  # csrc/common.h, the launchers in csrc/*.hip
SIZES = [1, 255, 256, 257, 2047, 2049, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 25) + 3]
NORMAL_MAX = 1 << 22  # random normal inputs up to here; integer inputs at every size
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def ints(rng, shape, dtype):
    return rng.integers(-8, 9, size=shape, dtype=np.int64).astype(NP[dtype])


def normal(rng, shape, dtype):
    return rng.standard_normal(shape, dtype=NP[dtype] if dtype == torch.float32 else np.float64)


def dev_t(a, dev):
    """A contiguous device copy (row-major strides also when the array is empty)."""
    a = np.ascontiguousarray(a)
    return torch.empty(a.shape, dtype=torch.from_numpy(a[:0]).dtype, device=dev).copy_(torch.from_numpy(a))


def host(t):
    return t.cpu().numpy()


def chunk(n, per_block, cap):
    """Elements per workgroup of a reduction with one contiguous chunk per workgroup."""
    grid = max(1, min(-(-n // per_block), cap))
    return -(-n // grid)


def agree(got, want, dtype, n, exact):
    """got (kernel, dtype) against want (float64): exactly float(want) cast to dtype, within the float64 tolerance of
    test_vector_ops, or within 1 ulp of float32(want)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if exact:
        assert np.array_equal(got, want.astype(NP[dtype]).astype(np.float64)), (got, want)
    elif dtype == torch.float64:
        assert np.max(np.abs(got - want)) < 1e-10 * np.sqrt(n), (got, want)
    else:
        w32 = want.astype(np.float32)
        assert np.all(np.abs(got - w32) <= np.spacing(np.abs(w32)).astype(np.float64)), (got, want)


def size_cases():
    return [(n, dtype, exact) for n in SIZES for dtype in DTYPES for exact in (True, False) if exact or n <= NORMAL_MAX]


@pytest.mark.parametrize("n,dtype,exact", size_cases())
def test_dots_and_probe_over_sizes(dev, n, dtype, exact):
    from odil_amd import ops

    rng = np.random.default_rng(n % 1000 + 7 * exact)
    gen = ints if exact else normal
    a, b, c = gen(rng, (2, n), dtype), gen(rng, n, dtype), gen(rng, n, dtype)
    a64, b64, c64 = (v.astype(np.float64) for v in (a, b, c))
    ta, tb, tc = dev_t(a, dev), dev_t(b, dev), dev_t(c, dev)
    agree(host(ops.dots(ta, tb)), a64 @ b64, dtype, n, exact)
    got = host(ops.dots3(ta, [tb, tc]))
    agree(got[:2], np.stack([a64 @ b64, a64 @ c64]), dtype, n, exact)
    assert np.all(got[2] == 0)
    out = torch.zeros(3, dtype=dtype, device=dev)
    ops.lbfgs_probe(tb, tc, out)
    got = host(out)
    agree(got[:2], [b64 @ c64, b64 @ b64], dtype, n, exact)
    assert got[2] == np.max(np.abs(b))  # exactly
    square = (b * b).astype(np.float64)  # (the kernel squares in the input precision)
    agree(float(ops.mean_reduce(tb)), square.sum() / n if exact else np.mean(square), dtype, n, exact)
    agree(float(ops.mean_reduce(tb, square=False)), b64.sum() / n if exact else np.mean(b64), dtype, n, exact)
    got = host(ops.max_abs_diff(tb, tc))
    assert got[0] == np.max(np.abs(b64 - c64)).astype(NP[dtype]) and got[1] == np.max(np.abs(c))
    got = host(ops.max_abs_rows(ta))
    assert np.array_equal(got, np.max(np.abs(a), axis=1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvec", [1, 50, 100, 128, 129])
def test_dots3_both_paths(dev, dtype, nvec):
    """n on both sides of 256 * 64, multiples of the vector width or not, contiguous, padded (lda > n) and odd-strided
    rows, one or three right-hand vectors: integer inputs, so every path must give the exact products."""
    from odil_amd import ops

    V = 16 // np.dtype(NP[dtype]).itemsize
    edge = BLOCK * 64
    rng = np.random.default_rng(nvec)
    for n in (edge - V, edge - 1, edge, edge + 1, edge + V, 3 * edge + 5 * V):
        bs = [ints(rng, n, dtype) for _ in range(3)]
        tbs = [dev_t(b, dev) for b in bs]
        for pad in (0, V, 1):
            a = ints(rng, (nvec, n + pad), dtype)
            ta = dev_t(a, dev)[:, :n]
            want = np.stack([a[:, :n].astype(np.float64) @ b.astype(np.float64) for b in bs])
            agree(host(ops.dots3(ta, tbs)), want, dtype, n, True)
            agree(host(ops.dots(ta, tbs[0])), want[0], dtype, n, True)
            got = host(ops.dots3(ta, tbs[:1]))
            agree(got[0], want[0], dtype, n, True)
            assert np.all(got[1:] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dots3_once_path_loops(dev, dtype):
    """The path that reads the right-hand vectors once caps its grid at 1024 chunks of 256 * 4 packs: above that
    every workgroup takes several chunks (the last one partial)."""
    from odil_amd import ops

    V = 16 // np.dtype(NP[dtype]).itemsize
    n = 1024 * BLOCK * 4 * V * 2 + 3 * BLOCK * V + V  # two full rounds and part of a third
    rng = np.random.default_rng(3)
    a, bs = ints(rng, (3, n), dtype), [ints(rng, n, dtype) for _ in range(3)]
    want = np.stack([a.astype(np.float64) @ b.astype(np.float64) for b in bs])
    agree(host(ops.dots3(dev_t(a, dev), [dev_t(b, dev) for b in bs])), want, dtype, n, True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lincomb_bit_for_bit(dev, dtype):
    from odil_amd import ops

    t = NP[dtype]
    rng = np.random.default_rng(17)
    for n in (1, 257, 2049, (1 << 21) + 1):
        for nvec in (0, 1, 100):
            if nvec == 100 and n > 2049:
                continue
            for pad in (0, 3):
                a = rng.standard_normal((nvec, n + pad)).astype(t)
                coef = rng.standard_normal(nvec).astype(t)
                y0 = rng.standard_normal(n).astype(t)
                for beta in (0.0, 1.0, -0.375, 1.7):
                    acc = np.zeros(n, dtype=t) if beta == 0 else t(beta) * y0
                    for k in range(nvec):
                        acc = acc + coef[k] * a[k, :n]
                    ty = dev_t(np.full(n, np.nan, dtype=t) if beta == 0 else y0, dev)  # beta 0: y is not read
                    ops.lincomb(ty, beta, dev_t(a, dev)[:, :n], dev_t(coef, dev))
                    assert np.array_equal(host(ty), acc), (n, nvec, pad, beta)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nrows", [1, 64])
def test_max_abs_rows_and_diff_above_the_grid_cap(dev, dtype, nrows):
    from odil_amd import ops

    rng = np.random.default_rng(nrows)
    # above the grid cap: 2048 workgroups for one row, 65536 / 64 = 1024 per row for 64 rows
    n = GRID_CAP * PER_BLOCK + 2 * BLOCK + 1 if nrows == 1 else (1 << 21) + 2 * BLOCK + 1
    a = normal(rng, (nrows, n), dtype)
    assert np.array_equal(host(ops.max_abs_rows(dev_t(a, dev))), np.max(np.abs(a), axis=1))
    n = GRID_CAP * PER_BLOCK + 2 * BLOCK + 1
    x, y = normal(rng, n, dtype), normal(rng, n, dtype)
    got = host(ops.max_abs_diff(dev_t(x, dev), dev_t(y, dev)))
    assert got[0] == np.max(np.abs(x.astype(np.float64) - y)).astype(NP[dtype]) and got[1] == np.max(np.abs(y))


def test_narrow_widen_bit_for_bit(dev):
    """s = a / sqrt(msq) (narrow) and a * sqrt(msq) (widen) for msq > 0, s = a for msq NULL, 0 or < 0.  The positive
    msq are exact squares, so that any correctly rounded sqrt gives the scale NumPy forms."""
    from odil_amd import ops

    rng = np.random.default_rng(23)
    for n in (1, 257, (1 << 21) + 1):
        x = rng.standard_normal(n) * 3.0
        y0 = rng.standard_normal(n)
        for a in (1.0, -0.3):
            for msq in (None, 6.25, 0.015625, 0.0, -4.0):
                tm = None if msq is None else torch.tensor(msq, dtype=torch.float64, device=dev)
                root = np.sqrt(msq) if msq is not None and msq > 0 else 1.0
                s_narrow = a if msq is None else np.float64(a) / root
                s_widen = a if msq is None else np.float64(a) * root
                y32 = ops.narrow_scale(dev_t(x, dev), torch.empty(n, dtype=torch.float32, device=dev), a, tm)
                assert np.array_equal(host(y32), (s_narrow * x).astype(np.float32)), (n, a, msq)
                x32 = rng.standard_normal(n).astype(np.float32)
                ty = ops.widen_axpy(dev_t(y0, dev), dev_t(x32, dev), a, tm)
                assert np.array_equal(host(ty), y0 + s_widen * x32.astype(np.float64)), (n, a, msq)
        # round trip: the residual normalised, narrowed, widened back with the inverse scale
        tm = torch.tensor(6.25, dtype=torch.float64, device=dev)
        y32 = ops.narrow_scale(dev_t(x, dev), torch.empty(n, dtype=torch.float32, device=dev), 1.0, tm)
        back = host(ops.widen_axpy(torch.zeros(n, dtype=torch.float64, device=dev), y32, 1.0, tm))
        assert np.all(np.abs(back - x) <= (2.0**-24 + 2.0**-50) * np.abs(x))


def boundaries(n, per):
    return sorted({i for i in (0, per - 1, per, n - 1) if 0 <= i < n})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [257, (1 << 21) + 1, (1 << 22) + 2 * BLOCK + 1])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_entries(dev, dtype, n, bad):
    from odil_amd import ops

    rng = np.random.default_rng(31)
    base = [normal(rng, n, dtype) for _ in range(3)]
    d = normal(rng, n, dtype)
    per = {"dot": chunk(n, PER_BLOCK, DOT_PARTIALS), "mean": chunk(n, PER_BLOCK, GRID_CAP)}
    places = sorted(set(boundaries(n, per["dot"]) + boundaries(n, per["mean"])))
    for i in places:
        g = base[0].copy()
        g[i] = bad
        g64 = g.astype(np.float64)
        tg = dev_t(g, dev)
        with np.errstate(invalid="ignore", over="ignore"):
            want_dot = g64 @ d.astype(np.float64)
            want_sq = np.sum(g64 * g64)
            want_sum = np.sum(g64)

        def same(got, want, what):
            got = float(got)
            assert (np.isnan(got) and np.isnan(want)) or got == want, (what, i, got, want)

        # dots / dots3: only the row holding the entry is affected
        a = np.stack([base[1], g, base[2]])
        ta = dev_t(a, dev)
        td = dev_t(d, dev)
        got = host(ops.dots(ta, td))
        same(got[1], want_dot, "dots")
        assert np.all(np.isfinite(got[[0, 2]]))
        got = host(ops.dots3(ta, [td]))
        same(got[0, 1], want_dot, "dots3")
        assert np.all(np.isfinite(got[0, [0, 2]]))
        out = torch.zeros(3, dtype=dtype, device=dev)
        got = host(ops.lbfgs_probe(tg, td, out))
        same(got[0], want_dot, "probe <g, d>")
        same(got[1], want_sq, "probe <g, g>")
        same(got[2], np.abs(bad), "probe max |g|")  # NaN for a NaN, +Inf for either infinity
        same(ops.mean_reduce(tg), want_sq / n, "mean square")
        same(ops.mean_reduce(tg, square=False), want_sum / n, "mean")
        got = host(ops.max_abs_diff(tg, dev_t(base[1], dev)))
        same(got[0], np.abs(bad), "max_abs_diff")
        got = host(ops.max_abs_rows(ta))
        same(got[1], np.abs(bad), "max_abs_rows")
        assert np.array_equal(got[[0, 2]], np.max(np.abs(a[[0, 2]]), axis=1))
    # every entry NaN
    tg = torch.full((n,), float("nan"), dtype=dtype, device=dev)
    out = torch.zeros(3, dtype=dtype, device=dev)
    assert bool(torch.isnan(ops.lbfgs_probe(tg, tg, out)).all())
    assert bool(torch.isnan(ops.max_abs_rows(tg[None])).all())


@pytest.mark.parametrize("where", ["one", "all"])
def test_lbfgsb_does_not_converge_on_a_nan_gradient(dev, where):
    """The stopping test reads max |g| from lbfgs_probe before anything else: a gradient with NaN entries must not pass
    it as NORM_OF_PROJECTED_GRADIENT_<=_PGTOL with warnflag 0."""
    from odil_amd.optimizer import LbfgsVectors, lbfgsb_minimize

    n = 5000
    x = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=dev)

    def fg(v):
        g = v.clone()
        if where == "all":
            g.fill_(float("nan"))
        else:
            g[n // 3] = float("nan")
        return 0.5 * (v * v).sum(), g

    res = lbfgsb_minimize(x, fg, LbfgsVectors(n, 5, dev), maxiter=10, m=5, maxls=20, pgtol=1e-16, factr=0.0)
    assert not (res["warnflag"] == 0 and res["task"].startswith("CONVERGENCE")), res
