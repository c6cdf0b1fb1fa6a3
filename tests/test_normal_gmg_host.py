"""Host-side checks (no GPU) of the multigrid for the normal equations of several grid fields (odil_amd/gmg.py:
NormalGMG): the planner's offset pattern and index maps, the assembly rule of csrc/block_mg.hip (emulated in NumPy), the
prolongation per loc and the coarse patterns, all against the independent restatement tests/normal_gmg_np.py and explicit
scipy.sparse products -- mixed locations, 1-3 dimensions, odd and even extents, periodic rolls, damping."""

import math
import types

import normal_gmg_np as ng
import numpy as np
import pytest
import scipy.sparse as sp

from odil_amd import gmg
from odil_amd.core import Field

# (cshape, {key: loc}, [(group loc, [(key, shift)])]): the output groups of a synthetic operator
CASES = {
    "1d-mixed-odd": ((7,), {"u": "c", "w": "n"},
                     [("c", [("u", (0,)), ("u", (-1,)), ("w", (0,)), ("w", (1,))]), ("n", [("u", (0,)), ("u", (1,)), ("w", (0,))])]),
    "1d-mixed-even": ((8,), {"u": "c", "w": "n"},
                      [("n", [("u", (0,)), ("u", (1,)), ("w", (-1,)), ("w", (1,))]), ("c", [("w", (0,)), ("w", (1,))])]),
    "2d-darcy-like": ((6, 4), {"p": "cc", "qx": "nc", "qy": "cn"},
                      [("cc", [("qx", (0, 0)), ("qx", (1, 0)), ("qy", (0, 0)), ("qy", (0, 1))]),
                       ("nc", [("qx", (0, 0)), ("p", (0, 0)), ("p", (1, 0))]),
                       ("cn", [("qy", (0, 0)), ("p", (0, 0)), ("p", (0, 1))])]),
    "2d-nonsquare-periodic": ((5, 6), {"u": "cc", "v": "nc"},
                              [("cc", [("u", (0, 0)), ("u", (-1, 0)), ("u", (0, 1)), ("v", (1, 0))]),
                               ("nc", [("v", (0, 0)), ("u", (0, -1))]), ("cc", [("u", (0, 0))])]),
    "3d-mixed": ((4, 3, 4), {"a": "ncc", "b": "ccn", "c": "ccc"},
                 [("ncc", [("a", (0, 0, 0)), ("a", (-1, 0, 0)), ("a", (0, 1, 1)), ("c", (0, 0, 0)), ("b", (1, 0, 0))]),
                  ("ccc", [("c", (0, 0, 0)), ("b", (0, 0, 1)), ("b", (0, -1, 0)), ("a", (1, 0, 0))])]),
}


def field_shape(cshape, loc):
    return tuple(n + (1 if ch == "n" else 0) for n, ch in zip(cshape, loc))


def synthetic(name, seed=0, case=None):
    """(fake LinearizedOperator for the planner, restatement fields, restatement blocks); case: a CASES value not listed"""
    cshape, locs, groups = case or CASES[name]
    rng = np.random.default_rng(seed)
    fields = {k: (l, field_shape(cshape, l)) for k, l in locs.items()}
    blocks, opblocks, row0 = [], [], 0
    for g, (gloc, reads) in enumerate(groups):
        oshape = field_shape(cshape, gloc)
        for key, shift in reads:
            coeff = rng.standard_normal(oshape)
            blocks.append((g, key, shift, gloc, coeff))
            opblocks.append((row0, math.prod(oshape), "stencil", key, (coeff, shift, gloc, oshape)))
        row0 += math.prod(oshape)
    op = types.SimpleNamespace(
        domain=types.SimpleNamespace(ndim=len(cshape), cshape=cshape),
        key_to_field={k: Field(np.zeros(fields[k][1]), loc=l) for k, l in locs.items()},
        key_to_size={k: math.prod(fields[k][1]) for k in locs}, blocks=opblocks)
    return op, fields, blocks


def emulate_assembly(op, damp=0.0, dampdiag=0.0):
    """The finest level as NormalGMG forms it: the planner's terms through the rule of k_bmg_assemble."""
    terms, keys, shapes = gmg.normal_pattern(op)
    out = dict()
    for a, b, o, b1, b2, rmap, rshape in terms:
        sa = shapes[a]
        arr = out.setdefault((a, b, o), np.zeros(sa))
        r = [rmap[:sa[0]], rmap[sa[0]:sa[0] + sa[1]], rmap[sa[0] + sa[1]:]]
        c1, c2 = np.asarray(b1[4][0]).reshape(rshape), np.asarray(b2[4][0]).reshape(rshape)
        for j in np.ndindex(*sa):
            rr = (r[0][j[0]], r[1][j[1]], r[2][j[2]])
            if min(rr) >= 0:
                arr[j] += c1[rr] * c2[rr]
    for a in range(len(keys)):
        d = out.setdefault((a, a, (0, 0, 0)), np.zeros(shapes[a]))
        if damp or dampdiag:
            d[...] = (d + damp**2) * (1 + dampdiag**2)
    return out, shapes


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("damp,dampdiag", [(0.0, 0.0), (0.3, 0.2)])
def test_assembly_equals_mtm(name, damp, dampdiag):
    op, fields, blocks = synthetic(name)
    m = ng.m_matrix(fields, blocks)
    want = (m.T @ m).toarray()
    if damp or dampdiag:
        want = want + np.diag((np.diag(want) + damp**2) * (1 + dampdiag**2) - np.diag(want))
    # the restatement's own block-offset form
    rest = ng.normal_entries(fields, blocks, damp, dampdiag)
    shapes = [fields[k][1] for k in fields]
    np.testing.assert_allclose(ng.entries_matrix(shapes, rest).toarray(), want, rtol=0, atol=1e-13 * np.abs(want).max())
    # the planner + assembly rule of the product (canonical 3-D shapes)
    entries, shapes3 = emulate_assembly(op, damp, dampdiag)
    got = ng.entries_matrix(shapes3, entries).toarray()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13 * np.abs(want).max())
    # only the offsets that occur are stored, each at most once
    pad = (0,) * (3 - len(shapes[0]))
    assert {(a, b, pad + o) for a, b, o in rest} <= set(entries) | {(a, a, (0, 0, 0)) for a in range(len(shapes))}


@pytest.mark.parametrize("kind,n", [("c", 8), ("c", 2), ("n", 9), ("n", 3), (".", 5)])
def test_prolongation_per_loc(kind, n):
    code = {".": 0, "c": 1, "n": 2}[kind]
    nc = gmg.coarse_shape3((1, 1, n), (0, 0, code))[2]
    p = gmg.p1d(code, n, nc)
    np.testing.assert_array_equal(p, ng.p1d(kind, n).toarray())
    np.testing.assert_allclose(p.sum(axis=1), 1.0)  # constants are interpolated exactly
    if kind != "." and nc >= 2:
        # linear functions too, away from the walls (positions in fine cell widths: coarse centre 2 I + 1, fine i + 1/2)
        xc = np.arange(nc) * 2.0 + (1.0 if kind == "c" else 0.0)
        xf = np.arange(n) + (0.5 if kind == "c" else 0.0)
        inner = slice(1, n - 1)
        np.testing.assert_allclose((p @ xc)[inner], xf[inner])


@pytest.mark.parametrize("name", sorted(set(CASES) - {"1d-mixed-odd"}))  # (7 cells: nothing halves)
def test_galerkin_pattern_covers_ptap(name):
    op, fields, blocks = synthetic(name, seed=1)
    entries, shapes3 = emulate_assembly(op)
    cshape = op.domain.cshape
    # every level down to where no axis halves any more
    locs = [fields[k][0] for k in fields]
    plan = None
    for limit in (1, 4, 16, 64, 256, 10**9):
        plan = plan or gmg.plan_levels(cshape, locs, max_coarsest=limit)
    shapes, codes = plan
    a = ng.entries_matrix(shapes3, entries)
    for lvl, code in enumerate(codes):
        kinds = ["".join(".cn"[c] for c in cf) for cf in code]
        p = ng.p_level(shapes[lvl], kinds)
        ac = ng.galerkin(a, p)
        pattern = gmg.coarse_pattern(sorted(entries), shapes[lvl], shapes[lvl + 1], code)
        assert ng.offsets_of(shapes[lvl + 1], shapes[lvl + 1], ac) <= set(pattern)
        # the next level's entries: P^T A P restricted to the planned pattern reproduces it
        cols0 = np.cumsum([0] + [math.prod(s) for s in shapes[lvl + 1]])
        entries = dict()
        for (ea, eb, o) in pattern:
            entries[(ea, eb, o)] = np.zeros(shapes[lvl + 1][ea])
        dense = ac.toarray()
        for (ea, eb, o), arr in entries.items():
            for q in np.ndindex(*shapes[lvl + 1][ea]):
                t = tuple(x + y for x, y in zip(q, o))
                if all(0 <= v < n for v, n in zip(t, shapes[lvl + 1][eb])):
                    arr[q] = dense[cols0[ea] + np.ravel_multi_index(q, shapes[lvl + 1][ea]),
                                   cols0[eb] + np.ravel_multi_index(t, shapes[lvl + 1][eb])]
        np.testing.assert_allclose(ng.entries_matrix(shapes[lvl + 1], entries).toarray(), dense, atol=1e-12 * np.abs(dense).max())
        a = ac


def test_radius_two_stays_radius_two():
    # a radius-2 cell-node pattern on a large grid: every coarse offset of |o| <= 2 has |J - I| <= 2 (asserted in the set-up)
    for ca, cb in [(1, 1), (1, 2), (2, 1), (2, 2)]:
        nfa, nfb = (64 if ca == 1 else 65), (64 if cb == 1 else 65)
        nca, ncb = (32 if ca == 1 else 33), (32 if cb == 1 else 33)
        for o in range(-2, 3):
            offs = gmg.coarse_axis_offsets(ca, nfa, nca, cb, nfb, ncb, o)
            assert offs and max(abs(v) for v in offs) <= 2, (ca, cb, o, offs)


def test_level_plan():
    shapes, codes = gmg.plan_levels((1024, 1024), ["cc", "nc", "cn"])
    assert len(shapes) == 6 and sum(math.prod(s) for s in shapes[-1]) <= gmg.COARSEST_MAX_UNKNOWNS
    assert shapes[1] == [(1, 512, 512), (1, 513, 512), (1, 512, 513)] and codes[0] == [[0, 1, 1], [0, 2, 1], [0, 1, 2]]
    shapes, codes = gmg.plan_levels((9, 64, 64), ["ncc"] * 3)  # the odd axis is never halved
    assert all(s[0][0] == 10 for s in shapes) and all(c[0][0] == 0 for c in codes)
    assert gmg.plan_levels((3, 5), ["cc", "nc"]) is None            # nothing halves
    assert gmg.plan_levels((6, 250), ["cc"] * 20) is None            # stops short of the coarsest size
    assert len(gmg.plan_levels((4,), ["c"])[0]) == 2                 # at least two levels


def many_fields(nf):
    """A 3-D case of nf fields (locs cycling through ccc ... nnn): every field read by its own output group and by the next
    field's group."""
    locs = ["".join("cn"[(k >> (2 - d)) & 1] for d in range(3)) for k in range(8)]
    keys = ["f{}".format(k) for k in range(nf)]
    groups = [(locs[k % 8], [(keys[k], (0, 0, 0)), (keys[(k + 1) % nf], (0, 1, 0))]) for k in range(nf)]
    return (4, 2, 6), {key: locs[k % 8] for k, key in enumerate(keys)}, groups


def test_field_limit_of_the_kernels():
    # 8 fields is the largest level descriptor of csrc/block_mg.hip (kBmgMaxFields); one more and the operator does not
    # qualify: create returns None (the solve falls back to CG on the normal equations) before anything touches a device
    assert gmg.MAX_FIELDS == 8
    op8, _, _ = synthetic(None, case=many_fields(8))
    terms, keys, shapes = gmg.normal_pattern(op8)
    assert len(keys) == 8 and sorted({s for s in shapes}) == sorted({field_shape((4, 2, 6), l) for l in many_fields(8)[1].values()})
    op9, _, _ = synthetic(None, case=many_fields(9))
    assert len(gmg.normal_pattern(op9)[1]) == 9
    assert gmg.NormalGMG.create(op9) is None
    assert gmg.NormalGMG.create(op9, damp=0.5, dampdiag=0.1) is None
