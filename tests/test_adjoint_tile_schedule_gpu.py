"""The two-tier z schedule of the LDS-tile transposes (csrc/common.h: TierSched): long chunks of coarse planes first,
short ones at the end of the launch.

Where a chunk is cut does not enter the arithmetic of k_poisson_adjoint_tile / k_interp_adj_tile, so every plan must
give the bits of the separate kernels: odil_poisson_adjoint(_adam) followed by the first P^T (+ Adam of that level),
never the launch under test.  The host-side test walks the kernels' own decode (odil_tile_sched_units): every
(coarse plane, tile) is covered exactly once, and a plan with L == S is the single-tier list the launch had before."""

import numpy as np
import pytest
import torch

ALPHA, OMB1, OMB2, EPS = 0.01, 0.1, 0.001, 1e-7
CUTS = [(False, False), (True, False), (False, True)]

# (L, Zs, S) at Z = 12 coarse planes: one chunk; chunks of one plane; both tiers ragged; no long tier; Zs no multiple of S
PLANS_12 = [(12, 12, 12), (4, 8, 1), (5, 10, 3), (2, 0, 2), (7, 7, 5)]


def plans_for(Z):
    """The same five kinds of plan for another plane count."""
    if Z == 12:
        return PLANS_12
    L = max(2, Z // 2)
    return [(Z, Z, Z), (max(2, Z // 3), Z - Z // 3, 1), (L, L, L - 1), (2, 0, 2), (Z - 1, Z - 1, max(1, Z - 3))]


CASES = [(np.float64, (24, 40, 136)), (np.float64, (8, 32, 128)), (np.float32, (16, 32, 512))]
PARAMS = [
    pytest.param(dtype, fine, plan, cut, id="{}-{}-L{}_Zs{}_S{}-cut{}{}".format(
        np.dtype(dtype).name, "x".join(map(str, fine)), *plan, int(cut[0]), int(cut[1])))
    for dtype, fine in CASES for plan in plans_for(fine[0] // 2) for cut in CUTS
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def to(x, dev):
    return torch.tensor(np.ascontiguousarray(x), device=dev)


def make_inputs(dtype, fine, dev):
    coarse = tuple(n // 2 for n in fine)
    rng = np.random.default_rng(43)
    fu = to(rng.standard_normal(fine).astype(dtype), dev)
    r = np.random.default_rng(47)
    mk = lambda s, pos=False: to((np.abs(r.standard_normal(s)) if pos else r.standard_normal(s)).astype(dtype), dev)
    state = [mk(fine), mk(coarse), mk(fine), mk(coarse), mk(fine, True), mk(coarse, True)]  # x0 x1 m0 m1 v0 v1
    h2 = [dtype(v) for v in [0.25**2, 0.1**2, 0.3**2]]
    return fu, state, h2, dtype(2.0 / np.prod(fine))


def embed(a, cut, fill):
    """`a` with two more planes beyond every cut end of axis 0: the nearer one repeats the end plane (what the one-launch
    kernel reads beyond a cut end: the index clamped into the array), the farther one is `fill`.  On that array the
    planes of `a` have the interior stencil rows on z that a cut end gives them."""
    parts = []
    if cut[0]:
        parts += [torch.full_like(a[:1], fill), a[:1]]
    parts.append(a)
    if cut[1]:
        parts += [a[-1:], torch.full_like(a[:1], fill)]
    return torch.cat(parts).contiguous()


def inner(a, cut, nz):
    lo = 2 if cut[0] else 0
    return a[lo:lo + nz].contiguous()


_refs = {}


def reference(dtype, fine, cut, dev):
    """By the separate kernels, once per (dtype, shape, cut): (g0, g1) of the gradient-only call, (g1, x0, x1, m0, m1, v0,
    v1) of the call with both Adam updates.  The stencil adjoint has no cut argument: it runs on the embedded array."""
    from odil_amd import ops

    key = (np.dtype(dtype).name, fine, cut)
    if key in _refs:
        return _refs[key]
    fu, state, h2, scale = make_inputs(dtype, fine, dev)
    coarse = tuple(n // 2 for n in fine)
    fu_e = embed(fu, cut, 0.0)
    g0 = inner(ops.poisson_adjoint(fu_e, h2, scale), cut, fine[0])
    g1 = ops.interp_adj(g0, "ccc", coarse, cut=cut)
    x0, x1, m0, m1, v0, v1 = [t.clone() for t in state]
    x0e, m0e, v0e = embed(x0, cut, 1.0), embed(m0, cut, 1.0), embed(v0, cut, 1.0)
    g0e = torch.empty_like(fu_e)
    ops.poisson_adjoint_adam(fu_e, h2, scale, g0e, x0e, m0e, v0e, ALPHA, OMB1, OMB2, EPS)
    g1a = torch.empty(coarse, dtype=fu.dtype, device=dev)
    ops.interp_adj_adam(inner(g0e, cut, fine[0]), "ccc", coarse, g1a, x1, m1, v1, ALPHA, OMB1, OMB2, EPS, cut=cut)
    upd = [g1a, inner(x0e, cut, fine[0]), x1, inner(m0e, cut, fine[0]), m1, inner(v0e, cut, fine[0]), v1]
    _refs[key] = ((g0, g1), upd)
    return _refs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,fine,plan,cut", PARAMS)
def test_every_plan_gives_the_bits_of_the_separate_kernels(dev, dtype, fine, plan, cut, monkeypatch):
    """g0 (stored), g1 and x, m, v of both levels of the one-launch kernel under an explicit plan == the separate
    kernels, torch.equal; wall ends and the slab form (one cut end) alike."""
    from odil_amd import ops

    monkeypatch.setenv("ODIL_ADJ_ROWS", "0")
    (g0_ref, g1_ref), upd_ref = reference(dtype, fine, cut, dev)
    fu, state, h2, scale = make_inputs(dtype, fine, dev)
    coarse = tuple(n // 2 for n in fine)
    g0 = torch.full(fine, 7.0, dtype=fu.dtype, device=dev)
    g1 = torch.full(coarse, 7.0, dtype=fu.dtype, device=dev)
    ops.poisson_adjoint_transpose(fu, h2, scale, g1, g0=g0, cut=cut, plan=plan)
    assert torch.equal(g0, g0_ref)
    assert torch.equal(g1, g1_ref)
    x0, x1, m0, m1, v0, v1 = [t.clone() for t in state]
    g1 = torch.full(coarse, 7.0, dtype=fu.dtype, device=dev)
    ops.poisson_adjoint_transpose(fu, h2, scale, g1, g0=None, adam0=(x0, m0, v0), adam1=(x1, m1, v1), alpha=ALPHA,
                                  one_minus_b1=OMB1, one_minus_b2=OMB2, eps=EPS, cut=cut, plan=plan)
    for name, a, b in zip(["g1", "x0", "x1", "m0", "m1", "v0", "v1"], [g1, x0, x1, m0, m1, v0, v1], upd_ref):
        assert torch.equal(a, b), name


@pytest.mark.gpu
def test_plain_transpose_on_the_tile_kernel_with_a_two_tier_plan(dev, monkeypatch):
    """ops.interp_adj(..., "ccc") at a shape where the rule cuts k_interp_adj_tile's launch into two tiers, against the
    register-window kernel (ODIL_ADJ_TILE=0), bit for bit; with a cut end as well."""
    from odil_amd import _lib, ops

    fine = (144, 512, 512)
    coarse = tuple(n // 2 for n in fine)
    L, Zs, S = ops.adjoint_transpose_plan(fine, transpose_only=True)
    assert 0 < Zs < coarse[0] and S < L, (L, Zs, S)  # two tiers
    monkeypatch.setenv("ODIL_ADJ_ROWS", "0")
    monkeypatch.setenv("ODIL_ADJ_TILE", "1")
    assert _lib.load().odil_interp_adj_kind(_lib.i64(coarse), 3, b"ccc", 8) == 4  # the LDS-tile kernel
    gen = torch.Generator(device=dev)
    gen.manual_seed(59)
    g = torch.randn(fine, dtype=torch.float64, device=dev, generator=gen)
    for cut in [(False, False), (True, False)]:
        monkeypatch.setenv("ODIL_ADJ_TILE", "1")
        tiled = ops.interp_adj(g, "ccc", coarse, cut=cut)
        monkeypatch.setenv("ODIL_ADJ_TILE", "0")
        plain = ops.interp_adj(g, "ccc", coarse, cut=cut)
        assert torch.equal(tiled, plain), cut


SCHEDULES = [
    # (Z, Y, XS, L, Zs, S)
    (256, 32, 8, 16, 256, 16),   # 512^3: the single tier the launch had
    (256, 32, 8, 32, 224, 8),    # 512^3, two tiers
    (256, 32, 8, 64, 200, 4),    # long tier ragged
    (12, 3, 3, 5, 10, 3),        # few rows, few chunks: plain order
    (40, 3, 2, 4, 30, 3),        # few rows, >= 8 chunks: split in the (chunk, y, xs) order
    (70, 37, 3, 9, 50, 7),       # rows not a multiple of the XCD count (padding workgroups), both tiers ragged
    (12, 40, 1, 2, 0, 2),        # no long tier
    (9, 33, 2, 9, 9, 9),         # one chunk
]


def test_rule_plan_of_the_headline_shape_is_two_tier():
    """512^3 takes two tiers by the rule; a shape with under two rounds of units keeps its single tier."""
    from odil_amd import ops

    L, Zs, S = ops.adjoint_transpose_plan((512, 512, 512))
    assert 1 <= S < L <= 64 and 0 < Zs < 256
    L, Zs, S = ops.adjoint_transpose_plan((24, 40, 136))
    assert Zs == 12 and L == S


def test_units_cover_every_plane_and_tile_once():
    """The decode the kernels run, walked on the host for every workgroup: each (coarse plane, tile) exactly once,
    chunks no longer than their tier's length, long chunks before short ones within an XCD's list, rows of XCD k in its
    chunk of rows; the rule's own plan at 512^3 included."""
    from odil_amd import ops

    rule = ops.adjoint_transpose_plan((512, 512, 512))
    for Z, Y, XS, L, Zs, S in SCHEDULES + [(256, 32, 8) + tuple(rule)]:
        units = ops.tile_sched_units(Z, Y, XS, L, Zs, S)
        count = np.zeros((Z, Y, XS), dtype=np.int64)
        two_tier = 0 < Zs < Z and S < L
        for b, u in enumerate(units):
            if u is None:
                continue
            z0, z1, y, xs = u
            assert 0 <= z0 < z1 <= Z and 0 <= y < Y and 0 <= xs < XS
            if two_tier:
                assert (z1 <= Zs and z1 - z0 <= L and z0 % L == 0) or (z0 >= Zs and z1 - z0 <= S and (z0 - Zs) % S == 0)
            else:
                assert z1 - z0 <= L
            count[z0:z1, y, xs] += 1
            if Y >= 32:  # rows split over the XCDs
                rows = (Y + 7) // 8
                assert y // rows == b % 8
        assert (count == 1).all(), (Z, Y, XS, L, Zs, S)
        if Y >= 32:  # within an XCD: ascending z, so every long chunk comes before every short one
            for k in range(8):
                starts = [u[0] for u in units[k::8] if u is not None]
                assert starts == sorted(starts)


def test_equal_lengths_reproduce_the_single_tier_list():
    """L == S (whatever Zs) is the schedule of make_unit_sched_chunked(Z, Y, XS, L): chunk zc = planes [zc L, zc L + L),
    in the order x-segment fastest, then the XCD's rows, then chunk (restated here for the XCD-split case)."""
    from odil_amd import ops

    for Z, Y, XS, L in [(256, 32, 8, 16), (70, 37, 3, 9), (12, 40, 1, 2)]:
        rows = (Y + 7) // 8
        nch = (Z + L - 1) // L
        want = []
        for b in range(8 * nch * rows * XS):
            k, i = b % 8, b // 8
            xs, r = i % XS, i // XS
            y, zc = k * rows + r % rows, r // rows
            want.append((zc * L, min(zc * L + L, Z), y, xs) if y < Y else None)
        for Zs in (Z, 0, Z // 2 + 1):
            assert ops.tile_sched_units(Z, Y, XS, L, Zs, L) == want, (Z, Y, XS, L, Zs)
