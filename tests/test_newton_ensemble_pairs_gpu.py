"""Two smoothing sweeps per pass in the batched cycle of a Newton ensemble (odil_stencil_var_smooth2_batch,
`gmg.EnsembleLaunchGMG.pair_min_cells`) on the device.  Every comparison is bit for bit, and against code that does not
contain the new kernel: the single sweeps, and the cycle with pairs off.

1  kernel pins: every member of a padded pack equals two single sweeps on its own arrays (and the single pair), for every
   chunk length and from the zero start; canaries stay, inputs stay; a member computes the same bits alone and at another
   position of a permuted batch; an inactive member's output is untouched
2  whole cycles with pairs on against pairs off: x, history and outcome, for nu1 / nu2 in 1 ... 4
3  freezing: members that stop after different cycle counts equal their own B = 1 solves and the pairs-off ensemble
4  the public driver with the class attribute at 0 and at inf
5  one real size: 2 members of 64^3"""

import math

import numpy as np
import pytest
import torch
from test_newton_ensemble_launches_gpu import _run_without_dense
from test_newton_ensemble_stencil_gpu import CANARY, _api, canaries_intact, members_pack, padded_rows, random_members

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
PAD = 6  # (even: every member begins on a pack of two cells)
W1, W2 = 0.9, 0.6
CASES = [((64,), None), ((130,), 0), ((12, 20), None), ((6, 260), None), ((8, 6, 10), None), ((4, 4, 4), 0),
         ((5, 28, 132), None), ((16, 16, 16), 0)]
CASE_IDS = ["64", "130-periodic", "12x20", "6x260", "8x6x10", "4^3-periodic", "5x28x132", "16^3-periodic"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------ 1: kernel pins
class Pins:
    """Two single sweeps, and the single pair, on the members of one (shape, periodic, dtype): computed once, left unchanged."""

    nb = 5

    def __init__(self, shape, periodic, dtype, dev):
        from odil_amd import ops

        self.shape = shape
        self.pack = members_pack(shape, periodic, dtype, dev, self.nb)
        self.x = random_members(self.nb, shape, dtype, dev, 31)
        self.b = random_members(self.nb, shape, dtype, dev, 32)
        self.two, self.two_zero, self.pair, self.pair_zero = [], [], [], []
        for m in range(self.nb):
            c, x, b = self.pack[m].contiguous(), self.x[m].contiguous(), self.b[m].contiguous()
            for src, two, pair in ((x, self.two, self.pair), (None, self.two_zero, self.pair_zero)):
                y1 = ops.stencil_var_smooth(c, src, b, W1, torch.empty_like(b))
                two.append(ops.stencil_var_smooth(c, y1, b, W2, torch.empty_like(b)))
                pair.append(ops.stencil_var_smooth2(c, src, b, W1, W2, torch.empty_like(b)))


_pins = dict()


def pins(shape, periodic, dtype, dev):
    key = (shape, periodic, dtype)
    if key not in _pins:
        _pins[key] = Pins(shape, periodic, dtype, dev)
    return _pins[key]


def padded(members):
    """(base [B, cells + PAD] with canaries behind every member, the view [B, *shape] of the members)."""
    shape = tuple(members.shape[1:])
    base = padded_rows(members, PAD)
    return base, base[:, :math.prod(shape)].unflatten(1, shape)


def run_pair(ref, order, dev, zero, zc_hint, active=None):
    """The batched pair on the members `order` of the reference pack, everything padded with canaries: out [B, *shape]."""
    from odil_amd import ops

    shape, dtype, nb = ref.shape, ref.pack.dtype, len(order)
    cells, need = math.prod(shape), (2 * len(shape) + 1) * math.prod(shape)
    coeffs = padded_rows(ref.pack[order], PAD)
    xbase, x = padded(ref.x[order])
    bbase, b = padded(ref.b[order])
    obase = torch.full((nb, cells + PAD), CANARY, dtype=dtype, device=dev)
    out = obase[:, :cells].unflatten(1, shape)
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=dev)
    ops.stencil_var_smooth2_batch(coeffs, None if zero else x, b, W1, W2, out, active=act, zc_hint=zc_hint)
    assert canaries_intact(coeffs, need) and canaries_intact(xbase, cells) and canaries_intact(bbase, cells)
    assert canaries_intact(obase, cells), "padding between members was written"
    assert torch.equal(coeffs[:, :need], ref.pack[order].reshape(nb, -1)), "the coefficients were written"
    assert torch.equal(x, ref.x[order]) and torch.equal(b, ref.b[order]), "an input was written"
    return out


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,periodic", CASES, ids=CASE_IDS)
def test_batched_pair_equals_two_single_sweeps(dev, shape, periodic, dtype):
    ref = pins(shape, periodic, dtype, dev)
    everyone = list(range(ref.nb))
    for zero in (False, True):
        two, pair = (ref.two_zero, ref.pair_zero) if zero else (ref.two, ref.pair)
        for zc_hint in (0, 1, 3, 64):
            what = (shape, "zero" if zero else "x", zc_hint)
            got = run_pair(ref, everyone, dev, zero, zc_hint)
            for m in everyone:
                assert torch.equal(got[m], two[m]), (what, m, "two single sweeps")
                assert torch.equal(got[m], pair[m]), (what, m, "the single pair")
            # a member alone, and at another position of a permuted batch
            alone = run_pair(ref, [1], dev, zero, zc_hint)
            moved = run_pair(ref, [3, 4, 2, 0, 1], dev, zero, zc_hint)
            assert torch.equal(alone[0], two[1]) and torch.equal(moved[4], two[1]) and torch.equal(moved[0], two[3]), what
            # an inactive member: its output keeps the canary fill, the others their bits
            masked = run_pair(ref, [0, 1, 2], dev, zero, zc_hint, active=[1, 0, 1])
            assert bool((masked[1] == CANARY).all()), (what, "an inactive member was written")
            assert torch.equal(masked[0], two[0]) and torch.equal(masked[2], two[2]), what


# ----------------------------------------------------------------------------------------------------- 2: whole cycles
@pytest.fixture()
def pair_launches(monkeypatch):
    """The number of pair launches made so far (the cycle reaches the kernel through `ops`)."""
    from odil_amd import ops

    count, inner = [0], ops.stencil_var_smooth2_batch

    def counted(*args, **kw):
        count[0] += 1
        return inner(*args, **kw)

    monkeypatch.setattr(ops, "stencil_var_smooth2_batch", counted)
    return count


def solvers(pack, **kw):
    """(pairs on every launch level, pairs off) on the same coefficients."""
    from odil_amd import gmg

    on, off = gmg.EnsembleLaunchGMG.from_coeffs(pack, **kw), gmg.EnsembleLaunchGMG.from_coeffs(pack, **kw)
    on.pair_min_cells, off.pair_min_cells = 0, math.inf
    assert all(on.pair_eligible(l) == (on.shapes[l][-1] % 2 == 0) for l in range(on.nlaunch))
    assert not any(off.pair_eligible(l) for l in range(off.nlaunch))
    return on, off


def assert_same_solve(on, off, b, x0, what, **kw):
    """Both solvers from the same start: x, history (as far as a member wrote it) and outcome, bit for bit."""
    xon, xoff = x0.clone(), x0.clone()
    on.solve(b, xon, **kw)
    off.solve(b, xoff, **kw)
    assert torch.equal(xon, xoff), what
    assert np.array_equal(on.outcome, off.outcome), (what, on.outcome, off.outcome)
    for m in range(on.nbatch):
        n = 2 + int(on.outcome[m, 0])
        assert np.array_equal(on.history[m, :n], off.history[m, :n]), (what, m)
        assert on.status(m) == off.status(m), (what, m)
    return xon


CONFIGS = [((32, 32), None, 64, 2), ((16, 16, 16), 0, 64, 2), ((12, 20), None, None, 1)]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nu1,nu2", [(2, 2), (3, 3), (1, 4), (4, 1)], ids=["nu22", "nu33", "nu14", "nu41"])
@pytest.mark.parametrize("shape,periodic,tail_max_cells,nlaunch", CONFIGS, ids=["32^2", "16^3-periodic", "12x20"])
def test_cycles_with_pairs_equal_cycles_without(dev, pair_launches, shape, periodic, tail_max_cells, nlaunch, nu1, nu2, dtype):
    nb = 3
    pack = members_pack(shape, periodic, dtype, dev, nb, seed=9)
    on, off = solvers(pack, nu1=nu1, nu2=nu2, tail_max_cells=tail_max_cells)
    assert on.nlaunch == off.nlaunch == nlaunch and on.shapes == off.shapes
    b, x0 = random_members(nb, shape, dtype, dev, 21), random_members(nb, shape, dtype, dev, 22)
    for start in (0, 2):
        for maxcycles in (1, 4):
            before = pair_launches[0]
            on.solve(b, x0.clone(), tol=0.0, maxcycles=maxcycles, start=start)
            made = pair_launches[0] - before
            assert made > 0, "no pair was launched"
            off.solve(b, x0.clone(), tol=0.0, maxcycles=maxcycles, start=start)
            assert pair_launches[0] - before == made, "pairs off launched a pair"
            assert_same_solve(on, off, b, x0, (start, maxcycles), tol=0.0, maxcycles=maxcycles, start=start)
    # and down to a tolerance
    assert_same_solve(on, off, b, x0, "tol", tol=1e-8 if dtype == F64 else 1e-4, maxcycles=30, start=2)


# ---------------------------------------------------------------------------------------------------------- 3: freezing
def test_members_that_stop_at_different_cycles_with_pairs(dev, pair_launches):
    from odil_amd import gmg

    shape, nb, tol = (16, 16), 3, 1e-6
    # (the recipe of test_members_that_stop_at_different_cycles_equal_their_own_solves)
    pack = members_pack(shape, None, F64, dev, nb, seed=11, scale0=[1.0] * nb)
    b = random_members(nb, shape, F64, dev, 41)
    grid = (torch.arange(16, dtype=F64, device=dev) + 0.5) / 16
    b[1] = torch.sin(math.pi * grid)[:, None] * torch.sin(math.pi * grid)[None, :]
    b[2] = 0.0
    on, off = solvers(pack, tail_max_cells=64)
    x0 = random_members(nb, shape, F64, dev, 42)
    x = assert_same_solve(on, off, b, x0, "ensemble", tol=tol, maxcycles=30, start=2)
    counts = [int(k) for k in on.outcome[:, 0]]
    print("cycles per member", counts, "reasons", on.outcome[:, 1])
    assert len(set(counts)) >= 2 and (on.outcome[:, 1] == 0).all(), on.outcome
    assert pair_launches[0] > 0
    for m in range(nb):
        alone = gmg.EnsembleLaunchGMG.from_coeffs(pack[m:m + 1].contiguous(), tail_max_cells=64)
        alone.pair_min_cells = 0
        xm = random_members(1, shape, F64, dev, 43)
        alone.solve(b[m:m + 1].contiguous(), xm, tol=tol, maxcycles=30, start=2)
        assert torch.equal(xm[0], x[m]), m
        assert np.array_equal(alone.outcome[0], on.outcome[m]), (m, alone.outcome, on.outcome)
        n = 2 + counts[m]
        assert np.array_equal(alone.history[0, :n], on.history[m, :n]), m
        assert on.status(m) == alone.status(0)


# ----------------------------------------------------------------------------------------------------- 4: public driver
@pytest.fixture()
def small_tail(monkeypatch):
    from odil_amd import gmg

    monkeypatch.setattr(gmg.EnsembleLaunchGMG, "tail_max_cells", 64)


@pytest.mark.parametrize("spec", ["--ndim 2 --N 16 --kind smooth", "--ndim 3 --N 8 --kind smooth --double 0"], ids=["2d-f64", "3d-f32"])
def test_optimize_newton_ensemble_with_pairs_equals_without(dev, small_tail, pair_launches, monkeypatch, spec):
    from odil_amd import gmg

    odil, ensemble = _api()
    runs = []
    for threshold in (0, math.inf):
        monkeypatch.setattr(gmg.EnsembleLaunchGMG, "pair_min_cells", threshold)
        before = pair_launches[0]
        args, problems, states, _, seen, arrays, info = _run_without_dense(odil, ensemble, spec + " --linsolver multigrid", 3, 2,
                                                                           form="launches")
        assert info.form == "launches" and info.route == "stencil"
        assert (pair_launches[0] > before) == (threshold == 0)
        runs.append((states, seen, info))
    (son, seen_on, ion), (soff, seen_off, ioff) = runs
    assert son[0].fields["u"].array.dtype == (F32 if "--double 0" in spec else F64)
    assert np.array_equal(ion.cycles, ioff.cycles) and np.array_equal(ion.residuals, ioff.residuals)
    assert (ion.cycles >= 1).all()
    for b in range(3):
        assert torch.equal(son[b].fields["u"].array, soff[b].fields["u"].array), b
        assert [st for _, _, st, _ in seen_on[b]] == [st for _, _, st, _ in seen_off[b]], b
        assert [loss for _, loss, _, _ in seen_on[b]] == [loss for _, loss, _, _ in seen_off[b]], b


# ---------------------------------------------------------------------------------------------------- 5: one real size
def test_two_members_of_64_cubed(dev, pair_launches):
    shape, nb, tol = (64, 64, 64), 2, 1e-10
    pack = members_pack(shape, None, F64, dev, nb, seed=13)
    on, off = solvers(pack)
    assert on.nlaunch == 1 and on.pair_eligible(0)
    b = random_members(nb, shape, F64, dev, 51)
    assert_same_solve(on, off, b, torch.zeros_like(b), "64^3", tol=tol, maxcycles=60, start=2)
    print("64^3 cycles", on.outcome[:, 0], "pair launches", pair_launches[0])
    assert pair_launches[0] > 0
    assert all(on.status(m)["converged"] for m in range(nb)), [on.status(m) for m in range(nb)]
    assert np.array_equal(on.outcome[:, 0], off.outcome[:, 0])
