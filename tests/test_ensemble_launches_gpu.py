"""The ensemble of Poisson problems as batched launches -- odil_poisson_residual_batch, odil_poisson_adjoint_adam_batch,
odil_mg_synth_adj_adam_members, odil_mg_synth on [B, *shape] arrays (csrc/poisson.hip, csrc/mg_transfer.hip, csrc/mg_fast.hip),
fused.PoissonLaunchEnsemble, AdamNativeOptimizer.run_ensemble, util.optimize_ensemble(form="launches") -- against each
member's own loop of `PoissonEvaluator.loss_grad_arrays(adam=...)`: the launches a single `optimize_grad` run makes.

Member b of a batched launch runs the single kernel's per-thread arithmetic on its own arrays and its loss is summed in the
single launch's order, so the requirement is EXACT equality (torch.equal): x, m, v of every level, and every epoch's loss
and norm.

Grids (the smallest that reach each code path; level shapes fine -> coarse):
  2d-64      (64,64) -> (8,8), 4 levels   refused by the workgroup form in float64; power of two; 16-byte packs
  2d-36x50   (36,50), (18,25)             float32 rows no multiple of 4 (masked tail, FULL = false); odd coarse row
  2d-12x1040 (12,1040), (6,520)           a row longer than one workgroup's x segment (256 lanes x 16 bytes)
  1d-8192    (8192,) -> (512,), 5 levels  1-D above small_max_cells; 16 x segments; the '.c' transfer layout
  2d-16      (16,16) -> (2,2), 4 levels   tiny coarse levels: single and batched runs take the same kernel on every level
A member's single run is computed once per (grid, dtype, epochs, step size) and shared, unchanged, by the cases."""

import functools
import os
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT

pytestmark = pytest.mark.gpu

LR = 0.005
OMB1, OMB2, EPS = 1 - 0.9, 1 - 0.999, 1e-7
BMAX = 70

GRIDS = {
    "2d-64": ((64, 64), 4),
    "2d-36x50": ((36, 50), 2),
    "2d-12x1040": ((12, 1040), 2),
    "1d-8192": ((8192,), 5),
    "2d-16": ((16, 16), 4),
}
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def level_shapes(grid):
    cshape, nlvl = GRIDS[grid]
    return [tuple(n >> l for n in cshape) for l in range(nlvl)]


def member_lr(member, per_member):
    return 0.001 * (1 + member % 7) if per_member else LR


def step_sizes(dtype, lr, nepochs):
    """The step sizes of a run as AdamNativeOptimizer forms them (numbers of the working precision)."""
    from odil_amd.optimizer import _adam_step_size

    npdt = np.float64 if dtype == torch.float64 else np.float32
    return [_adam_step_size(npdt(lr), npdt(0.9), npdt(0.999), npdt(t)) for t in range(1, nepochs + 1)]


def step_table(dtype, lrs, nepochs):
    rows = np.array([step_sizes(dtype, lr, nepochs) for lr in lrs], dtype=np.float64)
    return torch.tensor(rows, dtype=dtype, device="cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(grid, dname):
    """(evaluators of BMAX members, their initial levels): seeded right-hand sides and guesses, all different, anisotropic h2."""
    from odil_amd import fused

    dtype, dev = DTYPES[dname], torch.device("cuda:0")
    npdt = np.float64 if dtype == torch.float64 else np.float32
    shapes = level_shapes(grid)
    cshape = shapes[0]
    gen = torch.Generator().manual_seed(11 + len(grid))
    rhs = torch.randn((BMAX,) + cshape, generator=gen, dtype=torch.float64).to(dtype).to(dev)
    x0 = [(0.1 * torch.randn((BMAX,) + s, generator=gen, dtype=torch.float64)).to(dtype).to(dev) for s in shapes]
    h2 = [npdt((1.0 + axis) / n) ** 2 for axis, n in enumerate(cshape)]
    evs = [fused.PoissonEvaluator(cshape, shapes, rhs[b].contiguous(), h2, dtype=dtype, device=dev) for b in range(BMAX)]
    return evs, x0


def adam_constants(dname, native):
    """(1 - beta_1, 1 - beta_2): the test's own numbers, or as AdamNativeOptimizer forms them in the working precision."""
    if not native:
        return OMB1, OMB2
    npdt = np.float64 if dname == "f64" else np.float32
    return float(1 - npdt(0.9)), float(1 - npdt(0.999))


@functools.lru_cache(maxsize=None)
def single_run(grid, dname, nepochs, per_member, member, native=False):
    """Member `member` alone: nepochs times the launches of `loss_grad_arrays(adam=...)` with host step sizes, as
    `optimize_grad` runs it eagerly.  (x, m, v level lists, losses [E], norms [E])."""
    evs, x0 = inputs(grid, dname)
    OMB1, OMB2 = adam_constants(dname, native)
    ev = evs[member]
    x = [t[member].clone() for t in x0]
    m, v = [torch.zeros_like(t) for t in x], [torch.zeros_like(t) for t in x]
    losses, norms = [], []
    for alpha in step_sizes(DTYPES[dname], member_lr(member, per_member), nepochs):
        loss, _ = ev.loss_grad_arrays(x, adam=(m, v, alpha, OMB1, OMB2, EPS))
        losses.append(loss.clone())
        norms.append(torch.sqrt(loss))
    losses, norms = torch.stack(losses), torch.stack(norms)
    assert bool(torch.isfinite(x[0]).all()) and bool((losses > 0).all())
    return x, m, v, losses, norms


def ensemble_of(grid, dname, ids, pad=0):
    from odil_amd import fused

    evs, x0 = inputs(grid, dname)
    ens = fused.PoissonLaunchEnsemble([evs[k] for k in ids], pad=pad)
    index = torch.tensor(list(ids), device="cuda:0")
    for dst, src in zip(ens.x, x0):
        dst.copy_(src[index])
    return ens


def table_of(dname, ids, nepochs, per_member):
    """[B, E] (per member) or [E] (shared) step sizes of the members `ids`."""
    table = step_table(DTYPES[dname], [member_lr(k, per_member) for k in ids], nepochs)
    return table if per_member else table[0].contiguous()


def run_epochs(ens, tables):
    out = []
    for table in tables:
        losses = torch.full((ens.nbatch, table.shape[-1]), -1.0, dtype=ens.dtype, device=ens.device)
        norms = torch.full_like(losses, -1.0)
        ens.epochs(table, losses, norms, OMB1, OMB2, EPS)
        out.append((losses, norms))
    return torch.cat([a for a, _ in out], dim=1), torch.cat([b for _, b in out], dim=1)


def assert_members_equal(ens, losses, norms, grid, dname, ids, nepochs, per_member, native=False):
    for pos, member in enumerate(ids):
        x, m, v, ref_losses, ref_norms = single_run(grid, dname, nepochs, per_member, member, native)
        for name, got, want in (("x", ens.levels(ens.x, pos), x), ("m", ens.levels(ens.m, pos), m),
                                ("v", ens.levels(ens.v, pos), v)):
            for lvl, (p, q) in enumerate(zip(got, want)):
                assert p.shape == q.shape and torch.equal(p, q), (
                    grid, dname, "member", member, "at", pos, name, "level", lvl, float((p - q).abs().max()))
        for name, got, want in (("losses", losses[pos], ref_losses), ("norms", norms[pos], ref_norms)):
            assert torch.equal(got, want), (grid, dname, "member", member, "at", pos, name, got.tolist(), want.tolist())


@pytest.mark.parametrize("nepochs", [1, 7])
@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("dname", ["f64", "f32"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_members_equal_single_runs_shared_step_sizes(grid, dname, nbatch, nepochs):
    ids = list(range(nbatch))
    ens = ensemble_of(grid, dname, ids)
    losses, norms = run_epochs(ens, [table_of(dname, ids, nepochs, False)])
    assert_members_equal(ens, losses, norms, grid, dname, ids, nepochs, False)


@pytest.mark.parametrize("dname", ["f64", "f32"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_members_equal_single_runs_per_member_lrs(grid, dname):
    """A [B, E] table: every member steps with its own lr, on every level, and equals the single run with that lr."""
    ids = [0, 1, 2]
    ens = ensemble_of(grid, dname, ids)
    losses, norms = run_epochs(ens, [table_of(dname, ids, 7, True)])
    assert_members_equal(ens, losses, norms, grid, dname, ids, 7, True)
    assert not torch.equal(ens.x[-1][0], ens.x[-1][1])


@pytest.mark.parametrize("grid", ["2d-64", "1d-8192"])
def test_seventy_members_and_the_position_of_a_member(grid):
    """B = 70, and a member's result does not depend on where it stands: member 0 at position 41 of 70 and at position
    0 of 3 (the case above) both equal its single run."""
    ids = list(range(1, 42)) + [0] + list(range(42, BMAX))
    assert len(ids) == BMAX and ids[41] == 0
    ens = ensemble_of(grid, "f64", ids)
    losses, norms = run_epochs(ens, [table_of("f64", ids, 7, True)])
    assert_members_equal(ens, losses, norms, grid, "f64", ids, 7, True)
    few = ensemble_of(grid, "f64", [0, 1, 2])
    few_losses, _ = run_epochs(few, [table_of("f64", [0, 1, 2], 7, True)])
    assert torch.equal(few_losses[0], losses[41])
    for a, b in zip(few.levels(few.x, 0), ens.levels(ens.x, 41)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("grid,dname,pad", [("2d-64", "f64", 6), ("2d-36x50", "f32", 4), ("1d-8192", "f32", 12)])
def test_member_strides_wider_than_a_member(grid, dname, pad):
    """fu, rhs, m[0], v[0] with `pad` elements (a multiple of 16 bytes) between the members: the members equal their single
    runs and the padding is not written.  (u, g and x of a PoissonLaunchEnsemble are also operands of the transfer chains,
    which take contiguous arrays: their strides are widened in the test of the two stencil launches below.)"""
    ids = [0, 1, 2]
    ens = ensemble_of(grid, dname, ids, pad=pad)
    cells = ens.cells
    assert ens.fu.stride(0) == cells + pad == ens.m[0].stride(0) == ens.v[0].stride(0) == ens.rhs.stride(0)
    losses, norms = run_epochs(ens, [table_of(dname, ids, 7, True)])
    assert_members_equal(ens, losses, norms, grid, dname, ids, 7, True)
    for t in (ens.fu, ens.m[0], ens.v[0], ens.rhs):
        rows = t.as_strided((3, cells + pad), (cells + pad, 1))
        assert bool((rows[:, cells:] == 0).all()), "padding between members was written"


@pytest.mark.parametrize("grid,dname", [("2d-64", "f64"), ("2d-36x50", "f32"), ("2d-12x1040", "f32"), ("1d-8192", "f64")])
def test_stencil_launches_with_every_member_stride_wider(grid, dname):
    """ops.poisson_residual_batch / poisson_adjoint_adam_batch with ALL their member strides wider than a member, each
    by another multiple of 16 bytes (u, rhs, fu; fu, g, x, m, v), against `ops.poisson_residual` / `poisson_adjoint_adam` on
    each member alone: fu, loss, g, x, m, v equal bit for bit and no padding is written."""
    from odil_amd import ops

    dtype, dev, nb = DTYPES[dname], torch.device("cuda:0"), 3
    evs, x0 = inputs(grid, dname)
    shape = evs[0].cshape
    cells, unit = evs[0].sizes[0], 16 // (8 if dname == "f64" else 4)
    gen = torch.Generator().manual_seed(5)

    def wide(k, values=None):
        """[nb, *shape] view with k packs of padding (filled with 777) after every member."""
        base = torch.full((nb, cells + k * unit), 777.0, dtype=dtype, device=dev)
        view = base[:, :cells].unflatten(1, shape) if len(shape) > 1 else base[:, :cells]
        if values is not None:
            view.copy_(values)
        return base, view

    rnd = lambda: torch.randn((nb,) + shape, generator=gen, dtype=torch.float64).to(dtype).to(dev)
    (ub, u), (rb, rhs), (fb, fu) = wide(1, rnd()), wide(2, rnd()), wide(3)
    (gb, g), (xb, x), (mb, m), (vb, v) = wide(4), wide(5, rnd()), wide(6, 0.1 * rnd()), wide(7, rnd().abs())
    x_in, m_in, v_in = x.clone(), m.clone(), v.clone()
    npart = ops.poisson_batch_partials(shape, dtype)
    partials = torch.full((nb, npart + 3), 777.0, dtype=torch.float64, device=dev)
    loss = torch.zeros(nb, dtype=dtype, device=dev)
    alphas = torch.tensor([0.001, 0.002, 0.003], dtype=dtype, device=dev)
    h2, scale = evs[0].h2, float(evs[0].scale)
    ops.poisson_residual_batch(u, rhs, h2, fu, loss, partials[:, :npart])
    ops.poisson_adjoint_adam_batch(fu, h2, scale, g, x, m, v, alphas, OMB1, OMB2, EPS)
    for b in range(nb):
        fu1, loss1 = ops.poisson_residual(u[b].contiguous(), rhs[b].contiguous(), h2)
        x1, m1, v1 = x_in[b].clone(), m_in[b].clone(), v_in[b].clone()
        g1 = ops.poisson_adjoint_adam(fu1, h2, scale, torch.empty_like(fu1), x1, m1, v1, float(alphas[b]), OMB1, OMB2, EPS)
        for name, got, want in (("fu", fu[b], fu1), ("loss", loss[b], loss1), ("g", g[b], g1), ("x", x[b], x1),
                                ("m", m[b], m1), ("v", v[b], v1)):
            assert torch.equal(got, want), (grid, dname, b, name)
    for k, base in enumerate((ub, rb, fb, gb, xb, mb, vb), start=1):
        assert bool((base[:, cells:] == 777.0).all()), ("padding written", k)
    assert bool((partials[:, npart:] == 777.0).all())


@pytest.mark.parametrize("grid,dname", [("2d-64", "f64"), ("2d-36x50", "f32"), ("1d-8192", "f64")])
def test_two_chunks_equal_one(grid, dname):
    """State and moments persist across calls: 3 + 4 epochs in two calls equal 7 in one (both kinds of table)."""
    ids = [0, 1, 2]
    for per_member in (False, True):
        ens = ensemble_of(grid, dname, ids)
        table = table_of(dname, ids, 7, per_member)
        losses, norms = run_epochs(ens, [table[..., :3], table[..., 3:]])
        assert_members_equal(ens, losses, norms, grid, dname, ids, 7, per_member)


@pytest.mark.parametrize("grid,dname", [("2d-64", "f64"), ("2d-12x1040", "f32")])
def test_run_to_run_reproducible(grid, dname):
    ids = list(range(BMAX))
    runs = []
    for _ in range(2):
        ens = ensemble_of(grid, dname, ids)
        runs.append((ens,) + run_epochs(ens, [table_of(dname, ids, 7, True)]))
    (a, la, na), (b, lb, nb) = runs
    for name in ("x", "m", "v", "g"):
        for p, q in zip(getattr(a, name), getattr(b, name)):
            assert torch.equal(p, q), name
    assert torch.equal(la, lb) and torch.equal(na, nb)


@pytest.mark.parametrize("per_member", [False, True], ids=["lr", "lrs"])
@pytest.mark.parametrize("grid,dname", [("2d-64", "f64"), ("1d-8192", "f32")])
def test_replayed_epochs_equal_eager_epochs(grid, dname, per_member, monkeypatch):
    """AdamNativeOptimizer.run_ensemble: ODIL_GRAPH=1 (two eager epochs, then the epoch replayed as a hipGraph, step sizes
    and the columns of the loss tables selected by the device index) equals ODIL_GRAPH=0, and both equal the single runs."""
    from odil_amd.optimizer import AdamNativeOptimizer

    ids, nepochs = [0, 1, 2], 12
    lrs = [member_lr(k, True) for k in ids] if per_member else None
    results = []
    for mode in ("0", "1"):
        monkeypatch.setenv("ODIL_GRAPH", mode)
        ens = ensemble_of(grid, dname, ids)
        seen = []
        x, info = AdamNativeOptimizer().run_ensemble(ens, nepochs, callback=lambda e, l, n: seen.append((e, l.clone(), n.clone())),
                                                     lr=LR, lrs=lrs, epsilon=EPS)
        assert [e for e, _, _ in seen] == list(range(1, nepochs + 1)) and info.evals == nepochs
        for e, l, n in seen:
            assert torch.equal(l, info.losses[:, e - 1]) and torch.equal(n, info.norms[:, e - 1])
        assert_members_equal(ens, info.losses, info.norms, grid, dname, ids, nepochs, per_member, native=True)
        results.append((x, info))
    (xa, ia), (xb, ib) = results
    assert torch.equal(ia.losses, ib.losses) and torch.equal(ia.norms, ib.norms)
    for ma, mb in zip(xa, xb):
        for p, q in zip(ma, mb):
            assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------- optimize_ensemble
def _api():
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    return odil, poisson


def _member(odil, poisson, spec, b, epochs):
    """Member b of a sweep over an examples/poisson problem: its own right-hand side and initial guess on every level."""
    args = poisson.parse_args(spec.split())
    args.epoch_start, args.epochs, args.lr = 0, epochs, LR
    problem, state = poisson.make_problem(args)
    problem.extra.rhs = problem.extra.rhs * (1.0 + 0.25 * b)
    gen = torch.Generator().manual_seed(100 + b)
    domain = problem.domain
    arrays = [0.05 * torch.randn(tuple(a.shape), generator=gen, dtype=torch.float64).to(a.device)
              for a in domain.arrays_from_state(state)]
    domain.arrays_to_state(arrays, state)
    return args, problem, state


@pytest.mark.parametrize("cadence", [None, 10], ids=["every-epoch", "every-10"])
@pytest.mark.parametrize("own_lrs", [False, True], ids=["lr", "lrs"])
def test_optimize_ensemble_launches_equals_optimize_grad(own_lrs, cadence, monkeypatch):
    """4 members of examples/poisson --ndim 2 --N 64, 30 epochs, form="launches": x, m, v of every member equal four
    `optimize_grad` runs exactly, the callbacks fire at the same epochs with equal losses and norms, and every member's
    state holds its result.  (The workgroup form refuses these members: 4096 cells in float64.)"""
    monkeypatch.setenv("ODIL_GRAPH", "0")
    odil, poisson = _api()
    spec, nb, epochs = "--ndim 2 --N 64", 4, 30
    lrs = [0.002, 0.005, 0.01, 0.02] if own_lrs else None

    def recorder(seen):
        def cb(state, epoch, pinfo):
            seen.append((epoch, float(np.array(pinfo["loss"])), float(np.array(pinfo["norms"][0]))))

        if cadence:
            cb.next_active = lambda epoch: (epoch // cadence + 1) * cadence
        return cb

    singles = []
    for b in range(nb):
        args, problem, state = _member(odil, poisson, spec, b, epochs)
        args.lr = lrs[b] if own_lrs else LR
        seen = []
        arrays, info = odil.util.optimize_grad(args, "adam", problem, state, recorder(seen))
        singles.append((seen, [a.clone() for a in arrays], [a.clone() for a in info.m], [a.clone() for a in info.v]))

    built = [_member(odil, poisson, spec, b, epochs) for b in range(nb)]
    args, problems, states = built[0][0], [p for _, p, _ in built], [s for _, _, s in built]
    with pytest.raises(ValueError, match="member 0: .*above the limit"):
        odil.util.optimize_ensemble(args, problems, states)
    seen = [[] for _ in range(nb)]
    per_member = [recorder(s) for s in seen]

    def callback(member, state, epoch, pinfo):
        assert state is states[member]
        per_member[member](state, epoch, pinfo)

    if cadence:
        callback.next_active = per_member[0].next_active
    arrays, info = odil.util.optimize_ensemble(args, problems, states, callback, lrs=lrs, form="launches")
    assert len(arrays) == nb and info.epochs == epochs and tuple(info.losses.shape) == (nb, epochs)
    want_epochs = [0] + (list(range(cadence, epochs + 1, cadence)) if cadence else list(range(1, epochs + 1)))
    for b in range(nb):
        ref_seen, x, m, v = singles[b]
        # (a single run of this size steps epoch by epoch and reports every epoch; the ensemble reports at the cadence)
        assert [e for e, _, _ in ref_seen] == list(range(epochs + 1))
        assert [e for e, _, _ in seen[b]] == want_epochs
        assert seen[b] == [r for r in ref_seen if r[0] in want_epochs], ("callbacks of member", b)
        final = problems[b].domain.arrays_from_state(states[b])
        for name, got, want in (("x", arrays[b], x), ("m", info.m[b], m), ("v", info.v[b], v), ("state", final, x)):
            assert len(got) == len(want) >= 2
            for lvl, (p, q) in enumerate(zip(got, want)):
                assert p.shape == q.shape and torch.equal(p, q), (b, name, lvl, float((p - q).abs().max()))
    assert not torch.equal(arrays[0][0], arrays[1][0])


def test_form_auto_on_small_members_is_the_workgroup_form():
    """1-D N = 256: `form="auto"` takes the one-workgroup epochs and gives the result of `form="workgroup"`; asked for,
    the launches form gives it too (both equal the single runs)."""
    odil, poisson = _api()
    results = {}
    for form in ("workgroup", "auto", "launches"):
        built = [_member(odil, poisson, "--ndim 1 --N 256", b, 20) for b in range(3)]
        arrays, info = odil.util.optimize_ensemble(built[0][0], [p for _, p, _ in built], [s for _, _, s in built], form=form)
        results[form] = [a.clone() for member in arrays for a in member] + [info.losses.clone(), info.norms.clone()]
        ran = type(getattr(info, "ensemble", None)).__name__  # (the launches form reports the ensemble it stepped)
        assert ran == ("PoissonLaunchEnsemble" if form == "launches" else "NoneType"), (form, ran)
    for form in ("auto", "launches"):
        for a, b in zip(results["workgroup"], results[form]):
            assert torch.equal(a, b), form
