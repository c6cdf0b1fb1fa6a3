"""The host-only layout of the slab driver for traced operators (odil_amd.slab_traced.SlabLayout) and the plan of the
optimizer's update inside the gathers (fused_update_plan): no GPU, no kernels.  Checked on every rank of every case:
the plane descriptors are the planes of the level arrays' views, the messages of two neighbours pair up, the update
covers every entry of the packed vector once, and the replicated ranges are the agglomerated levels."""

import functools
import itertools
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples", "wave"))

from slab_oracle_ops import PlaneList  # noqa: E402
from test_slab_traced_cpu import make_problem  # noqa: E402

from odil_amd.slab_traced import SlabLayout, fused_update_plan  # noqa: E402

PAIRS = [(2, 8), (3, 8), (4, 2), (2, 4), (8, 4)]  # (world, nx_rank); nx_rank 2, 4 leave agglomerated coarse levels
CASES = [(which, world, nx_rank, 1) for which in ("veltracer", "veltracer-factors", "veltracer3d") for world, nx_rank in PAIRS]
CASES.append(("wave", 2, 8, 0))  # a plain Field, cut along the LEADING axis: contiguous planes


@functools.lru_cache(maxsize=None)
def layouts(which, world, nx_rank, axis):
    """(the layouts of all ranks, the global domain, the global unknown arrays)."""
    if which == "wave":
        import odil_amd as odil
        import wave as ex

        odil.runtime._mod = odil.ModRocm(device="cpu")
        odil.util.set_log_file(open(os.devnull, "w"))
        problem, state = ex.make_problem(ex.parse_args(["--Nt", str(nx_rank * world), "--Nx", "8", "--multigrid", "0", "--double", "1"]))
    else:
        problem, state = make_problem(which, world, nx_rank)
    domain = problem.domain
    return [SlabLayout(domain, state, axis, r, world) for r in range(world)], domain, domain.arrays_from_state(state)


def views(lay, v):
    """[(level, view of the packed vector v, is the field's finest level)] of the arrays cut into slabs, in vector order."""
    return [(lv, v[pos:pos + cnt].view(shape), k == 0) for e in lay.entries for k, (pos, cnt, shape, lv) in enumerate(e.arrays())
            if lv is not None and not lv.replicated]


def packed(descs, v):
    return PlaneList(descs, "cpu").pack(v)


def planes(items):
    return torch.cat([lv.planes(a, pos).reshape(-1) for lv, a, pos in items] + [torch.zeros(0, dtype=torch.int64)])


@pytest.mark.parametrize("which,world,nx_rank,axis", CASES)
def test_descriptors_are_the_planes_of_the_views(which, world, nx_rank, axis):
    strided = False
    for lay in layouts(which, world, nx_rank, axis)[0]:
        v = torch.arange(lay.total)
        arrays = views(lay, v)
        assert arrays and {"lo": lay.rank > 0, "hi": lay.rank < world - 1} == {s: s in lay.x_send for s in ("lo", "hi")}
        for side in lay.x_send:
            own = lambda lv: 0 if side == "lo" else lv.n - 1
            ghost = lambda lv: -1 if side == "lo" else lv.n
            assert torch.equal(packed(lay.x_send[side], v), planes([(lv, a, own(lv)) for lv, a, _ in arrays]))
            assert torch.equal(packed(lay.x_recv[side], v), planes([(lv, a, ghost(lv)) for lv, a, _ in arrays]))
            for k in (0, 1):  # the finest levels, the coarser ones: ghost then own out, added to own then ghost
                mine = [(lv, a) for lv, a, top in arrays if top == (k == 0)]
                assert torch.equal(packed(lay.g_send[k][side], v),
                                   planes([(lv, a, pos(lv)) for lv, a in mine for pos in (ghost, own)]))
                assert torch.equal(packed(lay.g_add[k][side], v),
                                   planes([(lv, a, pos(lv)) for lv, a in mine for pos in (own, ghost)]))
            strided = strided or any(outer > 1 for _, outer, _, _ in lay.x_send[side])
    assert strided == (axis != 0)


@pytest.mark.parametrize("which,world,nx_rank,axis", CASES)
def test_messages_of_neighbours_pair_up(which, world, nx_rank, axis):
    lays = layouts(which, world, nx_rank, axis)[0]
    sizes = lambda descs: [outer * inner for _, outer, _, inner in descs]
    for lower, upper in zip(lays, lays[1:]):
        assert sizes(lower.x_send["hi"]) == sizes(upper.x_recv["lo"]) and sizes(upper.x_send["lo"]) == sizes(lower.x_recv["hi"])
        for k in (0, 1):
            assert sizes(lower.g_send[k]["hi"]) == sizes(upper.g_add[k]["lo"])
            assert sizes(upper.g_send[k]["lo"]) == sizes(lower.g_add[k]["hi"])
        assert sizes(lower.g_send[0]["hi"])


@pytest.mark.parametrize("which,world,nx_rank,axis", CASES)
def test_the_update_covers_every_entry_once(which, world, nx_rank, axis):
    for lay in layouts(which, world, nx_rank, axis)[0]:
        keys = [e.key for e in lay.entries if e.levels]
        subsets = [c for n in range(len(keys) + 1) for c in itertools.combinations(keys, n)]
        for subset, reread in itertools.product(subsets, ((), tuple(keys))):
            fused, post_flat, post_pieces = fused_update_plan(lay, subset, reread)
            assert set(fused) <= set(subset)
            count = torch.zeros(lay.total, dtype=torch.int64)
            for key, (first, last) in fused.items():  # the gather updates the owned planes first <= plane < last
                e = lay.by_key[key]
                lv = e.levels[0]
                assert (first, last) == (1, lv.n - 1)
                lv.planes(count[e.start:e.start + lv.size].view(lv.shape), first, last - first).add_(1)
            for lo, hi in post_flat:
                count[lo:hi] += 1
            for start, size, npieces, stride, offset, cnt in post_pieces:
                # ops.adam_step_pieces on the vectors' entries [start, start + size): elements o * stride + offset + j
                assert npieces == 0 or (npieces - 1) * stride + offset + cnt <= size
                for o in range(npieces):
                    count[start + o * stride + offset:start + o * stride + offset + cnt] += 1
            assert bool((count == 1).all()), (lay.rank, subset)
        # the skip rules: too few planes, an unknown the gathers read again, multigrid factors
        fused = fused_update_plan(lay, keys, ())[0]
        assert set(fused) == {k for k in keys if lay.by_key[k].levels[0].n >= 4 and not lay.by_key[k].factors}
        fused = fused_update_plan(lay, keys, keys)[0]
        assert all(lay.by_key[k].synthesised for k in fused)


@pytest.mark.parametrize("which,world,nx_rank,axis", CASES)
def test_replicated_ranges_and_unknown_counts(which, world, nx_rank, axis):
    lays, domain, global_arrays = layouts(which, world, nx_rank, axis)
    n_global = sum(int(a.numel()) for a in global_arrays)
    for lay in lays:
        want = [(pos, cnt) for e in lay.entries for pos, cnt, _, lv in e.arrays() if lv is not None and lv.replicated]
        assert lay.rep == want
        assert (len(lay.rep) > 0) == (which != "wave" and nx_rank < 8)
        whole = sum(cnt for e in lay.entries for _, cnt, _, lv in e.arrays() if lv is None or lv.replicated)
        assert whole == lays[0].n_unknowns_local - lays[0].n_owned
        index = lay.local_index()
        assert index.numel() == lay.n_unknowns_local and index.unique().numel() == index.numel()
        assert lay.local_cells * world == lay.global_cells == math.prod(domain.cshape)
    replicated = lays[0].n_unknowns_local - lays[0].n_owned
    assert sum(lay.n_unknowns_local for lay in lays) == n_global + (world - 1) * replicated
