"""The four kernels of the multigrid for the normal equations of several grid fields (csrc/block_mg.hip: odil_bmg_apply,
_assemble, _transfer, _galerkin), each in f64 and f32, called directly on hand-built levels and compared with float64
references from the restatement tests/normal_gmg_np.py and scipy.sparse -- never with another kernel's output:

  * apply     every mode against A x, b - A x, x + w D^-1 (b - A x) and w D^-1 b; seeded random levels of 1 to 8 fields
              in 1-3 dimensions, offsets in [-2, 2] and wrap offsets n - 1, fields without entries, totals below 256, at
              256 k +- 1 (field boundaries inside a thread block) and one of about 2^20 unknowns
  * transfer  restriction P^T f and prolongation add + P c per field and axis over every code and extent (code 0 of
              extent 1 and > 1, cells of coarse extent 1, 2, 3, 7, nodes of coarse extent 2, 3, 5), codes mixed across
              the fields of one launch; prolongation in place equals the out-of-place result bit for bit
  * galerkin  the coarse entries of gmg.coarse_pattern against P^T A P on random fine levels (code-0 axes, radius 2, wraps)
  * assemble  the rule restated by test_normal_gmg_host.emulate_assembly on its CASES (index maps with -1)
  * NormalGMG on shapes the other GPU tests skip: cells (12, 7) (one axis never halves) and a 3-D system at all eight
    locations (the 8-field limit); every level is the reference chain P^T A P and the multigrid solve matches the dense
    one.  Nine fields fall back to CG on the normal equations."""

import argparse
import functools
import math

import normal_gmg_np as ng
import numpy as np
import pytest
import torch
from test_normal_gmg_host import CASES, emulate_assembly, synthetic

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
TOL = {torch.float64: 1e-14, torch.float32: 2e-6}         # apply, transfer (relative to the summed magnitudes)
TOL_GALERKIN = {torch.float64: 1e-13, torch.float32: 2e-6}
KIND = ".cn"  # transfer code -> the restatement's kind


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rounded(a, dtype):
    """The float64 values the kernel sees for an input of `dtype`."""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if dtype == torch.float32 else a


def to(a, dtype, dev):
    return torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=dtype, device=dev)


def host(t):
    return t.double().cpu().numpy()


def check(got, want, scale, tol, what=""):
    """max |got - want| <= tol * max(scale): scale bounds the magnitude of the terms summed into each value"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    assert np.all(np.isfinite(got)), what
    err = float(np.max(np.abs(got - want))) if got.size else 0.0
    bound = tol * max(float(np.max(np.abs(scale))) if got.size else 0.0, 1e-300)
    assert err <= bound, (what, err, bound)


def pack(shapes, entries, dtype, dev):
    """A level as NormalGMG._pack lays it out: entries {(a, b, o): array over a's grid} sorted (a, b, o), one flat
    coefficient buffer, 8 int64 words per table entry, ebeg per field.  Returns (coef, table, desc, keys, starts)."""
    from odil_amd import gmg

    keys = sorted(entries)
    rows, starts, ebeg, pos = [], [], [0] * (len(shapes) + 1), 0
    for e, (a, b, o) in enumerate(keys):
        starts.append(pos)
        rows.append([a, b, o[0], o[1], o[2], pos, 0, 0])
        pos += math.prod(shapes[a])
        ebeg[a + 1] = e + 1
    for a in range(len(shapes)):
        ebeg[a + 1] = max(ebeg[a + 1], ebeg[a])
    coef = to(np.concatenate([np.asarray(entries[k]).reshape(-1) for k in keys]), dtype, dev)
    table = torch.tensor(rows, dtype=torch.int64, device=dev).reshape(-1)
    desc, offs = gmg.level_desc(shapes, ebeg)
    return coef, table, desc, keys, starts


def unpack(shapes, keys, starts, coef):
    return {k: coef[s:s + math.prod(shapes[k[0]])].reshape(shapes[k[0]]) for k, s in zip(keys, starts)}


def entries_abs(entries):
    return {k: np.abs(v) for k, v in entries.items()}


# ----------------------------------------------------------------------------------------------------------------------
# seeded random levels

def shape_for(rng, ndim, size=None, hi=9):
    """A canonical 3-D shape of `ndim` active axes (of `size` unknowns when given)."""
    if size is None:
        return (1,) * (3 - ndim) + tuple(int(v) for v in rng.integers(1, hi, ndim))
    if ndim == 1 or size < 4:
        return (1, 1, size)
    divs = [d for d in range(2, int(size ** 0.5) + 1) if size % d == 0]
    if not divs:
        return (1, 1, size)
    d = divs[len(divs) // 2]
    return (1, d, size // d) if ndim == 2 or size // d < 4 else shape_for(rng, 2, size // d)[1:] + (d,)


def random_entries(rng, shapes, ndim, per_field=(0, 5), empty=()):
    """{(a, b, o): coefficients over a's grid}: offsets in [-2, 2] on the active axes, some wrap offsets +-(n_b - 1);
    fields in `empty` (and some at random) have no entries.  Values where a + o leaves b's grid are random too (the
    kernels must skip them)."""
    nf = len(shapes)
    out = dict()
    for a in range(nf):
        if a in empty:
            continue
        for _ in range(int(rng.integers(*per_field))):
            b = int(rng.integers(nf))
            o = [0, 0, 0]
            for d in range(3 - ndim, 3):
                o[d] = int(rng.integers(-2, 3))
            if rng.random() < 0.3:
                d = int(rng.integers(3 - ndim, 3))
                o[d] = int(rng.choice([-1, 1])) * (shapes[b][d] - 1)
            out[(a, b, tuple(o))] = rng.standard_normal(shapes[a])
    if not out:
        out[(0, 0, (0, 0, 0))] = rng.standard_normal(shapes[0])
    return out


def apply_level(seed, ndim, nf, total=None):
    rng = np.random.default_rng(seed)
    if total is None:
        shapes = [shape_for(rng, ndim) for _ in range(nf)]
    else:
        shapes = [shape_for(rng, ndim, hi=max(3, int(round((total / nf) ** (1 / ndim))))) for _ in range(nf - 1)]
        rest = total - sum(math.prod(s) for s in shapes)
        assert rest >= 1, (total, shapes)
        shapes.append(shape_for(rng, ndim, size=rest))
    # (field 1 of several never has entries; field 0 of one field always some)
    entries = random_entries(rng, shapes, ndim, per_field=(0, 5) if total is None or total < 10**5 else (1, 3),
                             empty={1} if nf > 1 else ())
    return shapes, entries


# (seed, ndim, nf, total unknowns or None)
APPLY_CASES = [(0, 1, 1, None), (1, 1, 3, None), (2, 2, 2, None), (3, 2, 5, None), (4, 3, 8, None), (5, 3, 4, None),
               (6, 1, 2, 255), (7, 2, 6, 257), (8, 3, 8, 511), (9, 2, 3, 3 * 256 + 1), (10, 3, 7, 40 * 256 - 1),
               (11, 1, 8, 17 * 256 + 1), (12, 3, 3, (1 << 20) + 1)]


def apply_inputs(case, dtype):
    """Level, vectors and the float64 reference matrix of one APPLY_CASES row (inputs rounded to dtype)."""
    seed, ndim, nf, total = case
    shapes, entries = apply_level(*case)
    entries = {k: rounded(v, dtype) for k, v in entries.items()}
    n = sum(math.prod(s) for s in shapes)
    assert total is None or n == total
    rng = np.random.default_rng(seed + 1000)
    x, b = rounded(rng.standard_normal(n), dtype), rounded(rng.standard_normal(n), dtype)
    dinv = rounded(rng.uniform(0.1, 2.0, n), dtype)
    a = ng.entries_matrix(shapes, entries)
    aabs = ng.entries_matrix(shapes, entries_abs(entries))
    return shapes, entries, x, b, dinv, a, aabs


@pytest.mark.parametrize("case", APPLY_CASES, ids=["s{}-{}d-{}f-{}".format(*c[:3], c[3] or "small") for c in APPLY_CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_apply_every_mode(dev, case, dtype):
    from odil_amd import ops

    shapes, entries, x, b, dinv, a, aabs = apply_inputs(case, dtype)
    coef, table, desc, _, _ = pack(shapes, entries, dtype, dev)
    tx, tb, td = to(x, dtype, dev), to(b, dtype, dev), to(dinv, dtype, dev)
    omega = 0.7
    w = float(rounded(omega, dtype))
    ax, axabs = a @ x, aabs @ np.abs(x)
    y = torch.full_like(tx, float("nan"))
    tol = TOL[dtype]
    ops.bmg_apply(coef, table, desc, tx, y, mode=0)
    check(host(y), ax, axabs, tol, "mode 0")
    ops.bmg_apply(coef, table, desc, tx, y, b=tb, mode=1)
    check(host(y), b - ax, np.abs(b) + axabs, tol, "mode 1")
    ops.bmg_apply(coef, table, desc, tx, y, b=tb, dinv=td, mode=2, omega=omega)
    check(host(y), x + w * (dinv * (b - ax)), np.abs(x) + w * dinv * (np.abs(b) + axabs), tol, "mode 2")
    y.fill_(float("nan"))
    ops.bmg_apply(None, None, desc, None, y, b=tb, dinv=td, mode=3, omega=omega)
    check(host(y), w * (dinv * b), w * dinv * np.abs(b), tol, "mode 3")
    # the inputs are not written
    assert torch.equal(tx, to(x, dtype, dev)) and torch.equal(tb, to(b, dtype, dev))


# ----------------------------------------------------------------------------------------------------------------------
# transfers

# (code, coarse extent) per axis: every code and extent the planner produces, and the edges of each
AXIS_OPTIONS = [(0, 1), (0, 5), (1, 1), (1, 2), (1, 3), (1, 7), (2, 2), (2, 3), (2, 5)]


def fine_extent(code, nc):
    return nc if code == 0 else 2 * nc if code == 1 else 2 * nc - 1


def coverage_case(k):
    """nf = 1 + k % 8 fields; field f, axis d takes AXIS_OPTIONS[(k + f + 3 d) % 9]: over k = 0..8 every option occurs
    on every axis, and the fields of one launch mix codes."""
    nf = 1 + k % 8
    opts = [[AXIS_OPTIONS[(k + f + 3 * d) % 9] for d in range(3)] for f in range(nf)]
    codes = [[c for c, _ in of] for of in opts]
    coarse = [tuple(nc for _, nc in of) for of in opts]
    fine = [tuple(fine_extent(c, nc) for c, nc in of) for of in opts]
    return fine, coarse, codes


def sized_case(k, target, which):
    """Random codes and extents per field, then one code-0 field (1, 1, m) that brings the fine or coarse total to
    `target`."""
    rng = np.random.default_rng(100 + k)
    fine, coarse, codes, have = [], [], [], 0
    for _ in range(7):
        opts = [AXIS_OPTIONS[int(rng.integers(len(AXIS_OPTIONS)))] for _ in range(3)]
        cs = tuple(nc for _, nc in opts)
        fs = tuple(fine_extent(c, nc) for c, nc in opts)
        if have + math.prod(fs if which == "fine" else cs) > 0.8 * target:
            continue
        codes.append([c for c, _ in opts])
        coarse.append(cs)
        fine.append(fs)
        have += math.prod(fs if which == "fine" else cs)
    assert target > have, (target, have)
    fine.append((1, 1, target - have))
    coarse.append((1, 1, target - have))
    codes.append([0, 0, 0])
    return fine, coarse, codes


def big_case():
    """About 2^20 fine unknowns: cells halved on every axis, nodes, and a field halved on one axis only."""
    codes = [[1, 1, 1], [2, 2, 2], [0, 1, 0]]
    coarse = [(64, 64, 32), (33, 33, 17), (5, 16, 3)]
    fine = [tuple(fine_extent(c, nc) for c, nc in zip(cf, s)) for cf, s in zip(codes, coarse)]
    return fine, coarse, codes


TRANSFER_CASES = {"cover{}".format(k): functools.partial(coverage_case, k) for k in range(9)}
TRANSFER_CASES.update({"fine{}".format(t): functools.partial(sized_case, i, t, "fine")
                       for i, t in enumerate([255, 257, 4 * 256 - 1, 9 * 256 + 1])})
TRANSFER_CASES.update({"coarse{}".format(t): functools.partial(sized_case, 10 + i, t, "coarse")
                       for i, t in enumerate([511, 6 * 256 + 1])})
TRANSFER_CASES["big"] = big_case


def test_transfer_cases_cover_every_code_and_extent():
    seen, mixed = set(), 0
    for k in range(9):
        fine, coarse, codes = coverage_case(k)
        seen |= {(d, c, nc) for cf, s in zip(codes, coarse) for d, (c, nc) in enumerate(zip(cf, s))}
        mixed += all(len({cf[d] for cf in codes}) == 3 for d in range(3))
    assert seen == {(d, c, nc) for d in range(3) for c, nc in AXIS_OPTIONS}
    assert mixed >= 2  # launches whose fields take all three codes on every axis


@functools.lru_cache(maxsize=None)
def transfer_p(name):
    fine, coarse, codes = TRANSFER_CASES[name]()
    p = ng.p_level(fine, ["".join(KIND[c] for c in cf) for cf in codes])
    assert p.shape == (sum(math.prod(s) for s in fine), sum(math.prod(s) for s in coarse))
    return fine, coarse, codes, p


@pytest.mark.parametrize("name", list(TRANSFER_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_transfer_against_p(dev, name, dtype):
    from ctypes import c_int

    from odil_amd import gmg, ops

    fine, coarse, codes, p = transfer_p(name)
    pabs = abs(p)
    nfld = len(fine)
    fdesc, _ = gmg.level_desc(fine, [0] * (nfld + 1))
    cdesc, _ = gmg.level_desc(coarse, [0] * (nfld + 1))
    code = (c_int * (3 * nfld))(*[c for cf in codes for c in cf])
    rng = np.random.default_rng(7)
    nfine, ncoarse = p.shape
    f, c, add = (rounded(rng.standard_normal(n), dtype) for n in (nfine, ncoarse, nfine))
    tol = TOL[dtype]
    # restriction: P^T f
    out = torch.full((ncoarse,), float("nan"), dtype=dtype, device=dev)
    ops.bmg_restrict(fdesc, cdesc, code, to(f, dtype, dev), out)
    check(host(out), p.T @ f, pabs.T @ np.abs(f), tol, "restrict")
    # prolongation: add + P c, out of place and in place (as NormalGMG.prolong_add calls it)
    tc, tadd = to(c, dtype, dev), to(add, dtype, dev)
    out = torch.full((nfine,), float("nan"), dtype=dtype, device=dev)
    ops.bmg_prolong_add(fdesc, cdesc, code, tc, tadd, out)
    check(host(out), add + p @ c, np.abs(add) + pabs @ np.abs(c), tol, "prolong")
    assert torch.equal(tadd, to(add, dtype, dev))
    ops.bmg_prolong_add(fdesc, cdesc, code, tc, tadd, tadd)
    assert torch.equal(tadd, out)


# ----------------------------------------------------------------------------------------------------------------------
# Galerkin coarsening

def galerkin_level(seed):
    """A random fine level with a transfer as the planner makes them: 1 to 8 fields in 1-3 dimensions on one cell grid,
    per axis halved (cells of coarse extent m -> code 1, nodes of coarse extent m + 1 -> code 2) or not (code 0), per
    field and axis a random loc; radius-2 and wrap offsets, fields without entries."""
    rng = np.random.default_rng(200 + seed)
    ndim = 1 + seed % 3
    nf = int(rng.integers(1, 9)) if seed > 2 else (1, 4, 8)[seed]
    axes = [(False, 1)] * (3 - ndim)
    for d in range(ndim):
        halve = d != 0 or seed % 2 == 0  # (axis 0 of the active ones kept on odd seeds)
        axes.append((halve, int(rng.choice([1, 2, 3, 7]) if halve else rng.choice([1, 5]))))
    fine, coarse, codes = [], [], []
    for _ in range(nf):
        loc = [d >= 3 - ndim and rng.random() < 0.5 for d in range(3)]  # True: a node axis
        codes.append([0 if not h else 2 if node else 1 for (h, _), node in zip(axes, loc)])
        coarse.append(tuple(m + node for (_, m), node in zip(axes, loc)))
        fine.append(tuple((2 * m if h else m) + node for (h, m), node in zip(axes, loc)))
    entries = random_entries(rng, fine, ndim, per_field=(0, 5), empty={nf - 1} if nf > 2 else ())
    entries.setdefault((0, 0, (0, 0, 0)), rng.standard_normal(fine[0]))  # (as NormalGMG: the coarse table is not empty)
    return fine, coarse, codes, entries


GALERKIN_SEEDS = list(range(12))


@pytest.mark.parametrize("seed", GALERKIN_SEEDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_galerkin_against_ptap(dev, seed, dtype):
    from ctypes import c_int

    from odil_amd import gmg, ops

    fine, coarse, codes, entries = galerkin_level(seed)
    entries = {k: rounded(v, dtype) for k, v in entries.items()}
    nfld = len(fine)
    fcoef, ftable, fdesc, _, _ = pack(fine, entries, dtype, dev)
    centries = gmg.coarse_pattern(sorted(entries), fine, coarse, codes)
    assert centries
    dummy = {k: np.zeros(coarse[k[0]]) for k in centries}
    _, ctable, cdesc, ckeys, cstarts = pack(coarse, dummy, dtype, dev)
    assert ckeys == list(centries)
    total = sum(math.prod(coarse[a]) for a, _, _ in centries)
    ccoef = torch.full((total,), float("nan"), dtype=dtype, device=dev)
    code = (c_int * (3 * nfld))(*[c for cf in codes for c in cf])
    ops.bmg_galerkin(fdesc, cdesc, code, fcoef, ftable, ctable, len(centries), ccoef)
    got = unpack(coarse, ckeys, cstarts, host(ccoef))
    # the reference: P^T A P of the restatement
    p = ng.p_level(fine, ["".join(KIND[c] for c in cf) for cf in codes])
    want = ng.galerkin(ng.entries_matrix(fine, entries), p)
    scale = ng.galerkin(ng.entries_matrix(fine, entries_abs(entries)), abs(p))
    diff = (ng.entries_matrix(coarse, got) - want).toarray()
    check(diff, np.zeros_like(diff), scale.toarray(), TOL_GALERKIN[dtype], "P^T A P")
    # coefficients whose column lies outside b's coarse grid are written as zero
    for (a, b, o), arr in got.items():
        q = np.indices(coarse[a])
        t = q + np.array(o)[:, None, None, None]
        outside = ~np.all((t >= 0) & (t < np.array(coarse[b])[:, None, None, None]), axis=0)
        assert np.all(arr[outside] == 0), (a, b, o)


def test_galerkin_levels_cover_the_edges():
    """The random levels above include code-0 axes, radius-2 offsets, wrap offsets, fields without entries and 8 fields."""
    code0 = radius2 = wrap = empty = eight = False
    for seed in GALERKIN_SEEDS:
        fine, coarse, codes, entries = galerkin_level(seed)
        code0 |= any(c == 0 and n > 1 for cf, s in zip(codes, fine) for c, n in zip(cf, s))
        radius2 |= any(2 in map(abs, o) for _, _, o in entries)
        wrap |= any(abs(v) == fine[b][d] - 1 and abs(v) > 2 for _, b, o in entries for d, v in enumerate(o))
        empty |= any(all(k[0] != a for k in entries) for a in range(len(fine)))
        eight |= len(fine) == 8
    assert code0 and radius2 and wrap and empty and eight


# ----------------------------------------------------------------------------------------------------------------------
# assembly

@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_assemble_against_the_rule(dev, name, dtype):
    from odil_amd import gmg, ops

    op, _, _ = synthetic(name, seed=3)
    for blk in op.blocks:
        coeff = blk[4][0]
        coeff[...] = rounded(coeff, dtype)
    terms, keys, shapes = gmg.normal_pattern(op)
    assert any((rmap < 0).any() for *_, rmap, _ in terms)
    out = dict()
    for a, b, o, b1, b2, rmap, rshape in terms:
        arr = out.get((a, b, o))
        if arr is None:
            arr = out[(a, b, o)] = torch.full((math.prod(shapes[a]),), 0.0, dtype=dtype, device=dev)
        ops.bmg_assemble(to(b1[4][0], dtype, dev), to(b2[4][0], dtype, dev), torch.as_tensor(rmap, device=dev), shapes[a],
                         rshape, arr)
    want, _ = emulate_assembly(op)
    for blk in op.blocks:
        np.abs(blk[4][0], out=blk[4][0])
    scale, _ = emulate_assembly(op)
    for key, arr in want.items():
        got = host(out[key]).reshape(shapes[key[0]]) if key in out else np.zeros(shapes[key[0]])
        check(got, arr, scale[key], TOL[dtype], key)
    assert set(out) <= set(want)


# ----------------------------------------------------------------------------------------------------------------------
# through NormalGMG

def locs_problem(nf, cshape=(8, 4, 6)):
    """A 3-D system of nf fields, field k at the k-th of the eight locations ccc ... nnn (cycling): per field the rows
    f_k - 0.5 f_(k+1) (f_(k+1) read at f_k's loc) and the differences f_k(+1) - f_k along axis k % 3 -- M is not square,
    M^T M >= 0.25 I."""
    import odil_amd as odil

    locs = ["".join("cn"[(k >> (2 - d)) & 1] for d in range(3)) for k in range(8)]
    keys = ["f{}".format(k) for k in range(nf)]
    domain = odil.Domain(cshape=cshape, dimnames=["x", "y", "z"], lower=(0, 0, 0), upper=cshape, dtype=np.float64,
                         multigrid=0)
    rng = np.random.default_rng(9)
    rhs = [domain.mod.cast(rng.standard_normal(tuple(n + (ch == "n") for n, ch in zip(cshape, locs[k % 8]))), domain.dtype)
           for k in range(nf)]

    def operator(ctx):
        res = []
        for k, key in enumerate(keys):
            loc = locs[k % 8]
            nxt = ctx.field(keys[(k + 1) % nf], loc=loc)
            res.append(ctx.field(key) - 0.5 * nxt - rhs[k])
            shift = tuple(1 if d == k % 3 else 0 for d in range(3))
            res.append(ctx.field(key, *shift) - ctx.field(key))
        return res

    state = odil.State(fields={key: odil.Field(None, loc=locs[k % 8]) for k, key in enumerate(keys)})
    state = domain.init_state(state)
    return odil.Problem(operator, domain), state


def linearized(problem, state, seed=0):
    rng = np.random.default_rng(seed)
    arrays = [torch.as_tensor(rng.standard_normal(tuple(a.shape)) * 0.1, dtype=a.dtype).to(a.device)
              for a in problem.domain.arrays_from_state(state)]
    problem.domain.arrays_to_state(arrays, state)
    return problem.linearize_device(state)


def uc_ufx_12x7():
    import os

    import odil_amd as odil
    from test_normal_gmg_gpu import uc_ufx_problem

    odil.util.set_log_file(open(os.devnull, "w"))
    return uc_ufx_problem(12, 7)


def eight_locations():
    import os

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    return locs_problem(8)


def dense_reference(op, vector):
    """(M^T M, the solution of M^T M x = -M^T r) in float64 on the host."""
    m = op.to_dense().double().cpu().numpy()
    a = m.T @ m
    return a, np.linalg.solve(a, m.T @ (-vector.double().cpu().numpy()))


def solve_multigrid(op, vector):
    import odil_amd as odil

    args = argparse.Namespace(linsolver_tol=1e-13, linsolver_maxiter=None, linsolver_damp=0, linsolver_dampdiag=0)
    status = dict()
    x = odil.linsolver.solve(op, -vector, args, status, "multigrid")
    return x.double().cpu().numpy(), status


@pytest.mark.parametrize("make", [uc_ufx_12x7, eight_locations], ids=["uc_ufx-12x7", "eight-locations"])
def test_normal_gmg_on_uncovered_shapes(make):
    from odil_amd import gmg

    problem, state = make()
    vector, op = linearized(problem, state)
    solver = gmg.NormalGMG.create(op)
    assert solver is not None and solver.nlvl >= 2
    if make is eight_locations:
        assert solver.nf == gmg.MAX_FIELDS == 8
        assert sorted(op.key_to_field[k].loc for k in solver.keys) == sorted(
            a + b + c for a in "cn" for b in "cn" for c in "cn")
    else:
        assert solver.shapes[0] == [(1, 12, 7), (1, 13, 7)] and all(cf[2] == 0 for cf in solver.codes[0])
    a, want = dense_reference(op, vector)
    # every level against the reference chain: A_0 = M^T M, A_(l+1) = P^T A_l P of the restatement's P
    ref = a
    for lvl in range(solver.nlvl):
        if lvl:
            kinds = ["".join(KIND[c] for c in cf) for cf in solver.codes[lvl - 1]]
            p = ng.p_level(solver.shapes[lvl - 1], kinds).toarray()
            ref = p.T @ ref @ p
        got = solver.dense(lvl)
        assert np.abs(got - ref).max() <= (1e-14 if lvl == 0 else 1e-13) * np.abs(ref).max(), lvl
    x, status = solve_multigrid(op, vector)
    assert status["method"].startswith("gmg-normal"), status
    assert np.abs(x - want).max() <= 1e-9 * np.abs(want).max(), status


def test_nine_fields_fall_back_to_cg():
    """One field more than the kernels take (kBmgMaxFields): the multigrid route declines and CG on the normal equations
    solves the system (it used to raise OdilHipError from the first Galerkin launch)."""
    import os

    import odil_amd as odil
    from odil_amd import gmg

    odil.util.set_log_file(open(os.devnull, "w"))
    problem, state = locs_problem(9)
    vector, op = linearized(problem, state)
    assert len(op.key_to_field) == 9 and gmg.NormalGMG.create(op) is None
    a, want = dense_reference(op, vector)
    x, status = solve_multigrid(op, vector)
    assert not status.get("method", "").startswith("gmg"), status
    assert np.abs(x - want).max() <= 1e-9 * np.abs(want).max(), status
