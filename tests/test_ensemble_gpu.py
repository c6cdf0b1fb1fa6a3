"""The ensemble of small Poisson problems -- odil_poisson_small_epochs_batch (csrc/epoch_small.hip), fused.PoissonEnsemble,
AdamNativeOptimizer.run_ensemble, util.optimize_ensemble -- against the single-problem launch odil_poisson_small_epochs,
which tests/test_trajectories.py pins bit for bit to the multi-launch path and the goldens.

Workgroup b of the batched launch runs the per-workgroup code of the single launch on member b's pointers, so the
requirement is EXACT equality (torch.equal), not a tolerance: for every member, x, m, v, the gradient and the [E] losses
and norms after E epochs equal a single-problem run from the same inputs.

Grids (the smallest at which each form can still go wrong):
  1d-256    1-D N = 256, 8 levels (BASELINE config 1), LDS-resident, 256 threads
  1d-64     1-D N = 64, 6 levels
  2d-16     2-D 16^2, 4 levels, resident: rows and columns both coarsen
  2d-40x94  2-D 40 x 94, 2 levels (tests/test_poisson_grids_gpu.py): float64 runs from GLOBAL memory (admitted with
            `small_force`, as there), float32 is resident; x = 94 / 47 is no power of two (float quotient in small_row)
  2d-12x94  2-D 12 x 94, 2 levels, resident in both precisions, the float quotient undershoots (same file)
  2d-64x96  2-D 64 x 96, 3 levels: global memory in float32 too (one case, so that this instantiation runs)
None of the 2-D small cases of tests/test_poisson_grids_gpu.py has an odd number of rows on any level (levels halve
exactly), so there is no odd-row shape to add.
B = 1, 3 and 300 members (more than the 256 compute units: some take a second workgroup), E = 1 and 37 epochs, members
that differ in right-hand side and initial guess, one table of step sizes shared by all members and one row per member.
The single-problem reference of a (grid, dtype, E, table) is computed once for 300 members and shared, unchanged, by
the cases that need it."""

import argparse
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT

pytestmark = pytest.mark.gpu

BMAX = 300
LR = 0.005
OMB1, OMB2, EPS = 1 - 0.9, 1 - 0.999, 1e-7

# name -> (cshape, levels, needs small_force in float64)
GRIDS = {
    "1d-256": ((256,), 8),
    "1d-64": ((64,), 6),
    "2d-16": ((16, 16), 4),
    "2d-40x94": ((40, 94), 2),
    "2d-12x94": ((12, 94), 2),
    "2d-64x96": ((64, 96), 3),
}
MAIN = ["1d-256", "1d-64", "2d-16", "2d-40x94", "2d-12x94"]
DTYPES = {"f64": torch.float64, "f32": torch.float32}
# (grid, dtype) -> the state is resident in LDS
RESIDENT = {(g, d): True for g in GRIDS for d in DTYPES}
RESIDENT.update({("2d-40x94", "f64"): False, ("2d-64x96", "f64"): False, ("2d-64x96", "f32"): False})


def level_shapes(grid):
    cshape, nlvl = GRIDS[grid]
    return [tuple(n >> l for n in cshape) for l in range(nlvl)]


def step_table(dtype, lrs, nepochs):
    """[len(lrs), nepochs] step sizes as AdamNativeOptimizer forms them."""
    from odil_amd.optimizer import _adam_step_size

    npdt = np.float64 if dtype == torch.float64 else np.float32
    rows = [[_adam_step_size(npdt(lr), npdt(0.9), npdt(0.999), npdt(t)) for t in range(1, nepochs + 1)] for lr in lrs]
    return torch.tensor(np.array(rows, dtype=np.float64), dtype=dtype, device="cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(grid, dname):
    """(evaluators of BMAX members, x0 [BMAX, unknowns]): seeded right-hand sides and initial guesses, all different."""
    from odil_amd import fused

    dtype, dev = DTYPES[dname], torch.device("cuda:0")
    npdt = np.float64 if dtype == torch.float64 else np.float32
    shapes = level_shapes(grid)
    cshape = shapes[0]
    gen = torch.Generator().manual_seed(7 + len(grid))
    rhs = torch.randn((BMAX,) + cshape, generator=gen, dtype=torch.float64).to(dtype).to(dev)
    x0 = (0.1 * torch.randn((BMAX, sum(math.prod(s) for s in shapes)), generator=gen, dtype=torch.float64)).to(dtype).to(dev)
    h2 = [npdt((1.0 + axis) / n) ** 2 for axis, n in enumerate(cshape)]  # (anisotropic: another step per axis)
    evs = []
    for b in range(BMAX):
        ev = fused.PoissonEvaluator(cshape, shapes, rhs[b], h2, dtype=dtype, device=dev)
        ev.small_force = not RESIDENT[(grid, dname)] and len(cshape) == 2  # (as tests/test_poisson_grids_gpu.py admits them)
        evs.append(ev)
    return evs, x0


def single_run(ev, x0, tables):
    """Member `ev` alone through odil_poisson_small_epochs, one launch per table in turn: (x, m, v, g, losses, norms)."""
    x, m, v = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)
    levels = lambda t: [a.view(s) for a, s in zip(t.split(ev.sizes), ev.shapes)]
    heads = ev.small_plan(levels(x), levels(m), levels(v))
    assert heads is not None, "small_plan does not admit the grid"
    out = []
    for table in tables:
        losses, norms = torch.empty_like(table), torch.empty_like(table)
        ev.small_epochs(heads, table, losses, norms, OMB1, OMB2, EPS)
        out.append((losses, norms))
    return x, m, v, ev.g.clone(), torch.cat([a for a, _ in out]), torch.cat([b for _, b in out])


@functools.lru_cache(maxsize=None)
def reference(grid, dname, nepochs, per_member):
    """BMAX single-problem runs: dict of stacked x, m, v, g [BMAX, unknowns], losses, norms [BMAX, E], table [BMAX, E]."""
    evs, x0 = inputs(grid, dname)
    lrs = [0.001 * (1 + b % 7) for b in range(BMAX)] if per_member else [LR] * BMAX
    table = step_table(DTYPES[dname], lrs, nepochs)
    runs = [single_run(ev, x0[b], [table[b]]) for b, ev in enumerate(evs)]
    ref = {name: torch.stack([r[k] for r in runs]) for k, name in enumerate(("x", "m", "v", "g", "losses", "norms"))}
    ref["table"] = table
    assert bool(torch.isfinite(ref["x"]).all()) and bool((ref["losses"] > 0).all())
    return ref


def ensemble_of(grid, dname, nbatch):
    from odil_amd import fused

    evs, x0 = inputs(grid, dname)
    ens = fused.PoissonEnsemble(evs[:nbatch])
    ens.x.copy_(x0[:nbatch])
    return ens


def run_ensemble(ens, tables):
    """One batched launch per table ([E] shared or [B, E]) in turn: the [B, sum E] losses and norms."""
    out = []
    for table in tables:
        losses = torch.full((ens.nbatch, table.shape[-1]), -1.0, dtype=ens.dtype, device=ens.device)
        norms = torch.full_like(losses, -1.0)
        ens.epochs(table, losses, norms, OMB1, OMB2, EPS)
        out.append((losses, norms))
    return torch.cat([a for a, _ in out], dim=1), torch.cat([b for _, b in out], dim=1)


def assert_members_equal(ens, losses, norms, ref, what):
    nb = ens.nbatch
    got = dict(x=ens.x, m=ens.m, v=ens.v, g=ens.g, losses=losses, norms=norms)
    for name, t in got.items():
        want = ref[name][:nb]
        if not torch.equal(t, want):
            rows = (t != want).flatten(1).any(dim=1).nonzero().flatten().tolist()
            raise AssertionError("{}: {} of members {} differ from their single runs (max |d| {:.3g})".format(
                what, name, rows[:8], float((t - want).abs().max())))


def test_the_grids_cover_both_forms():
    """The cases above run what their comments say: resident / global-memory as odil_poisson_small_epochs_resident decides,
    and small_plan's predicate admits every one of them (the global-memory 2-D ones with small_force)."""
    from odil_amd import fused
    from odil_amd._lib import i64, load

    forms = set()
    for (grid, dname), want in RESIDENT.items():
        shapes = level_shapes(grid)
        flat = [n for s in shapes for n in s]
        got = bool(load().odil_poisson_small_epochs_resident(i64(flat), len(shapes), len(shapes[0]), 8 if dname == "f64" else 4))
        assert got == want, (grid, dname)
        assert fused.small_refusal(shapes, DTYPES[dname], force=not want) is None, (grid, dname)
        forms.add((dname, got))
    assert forms == {("f64", True), ("f64", False), ("f32", True), ("f32", False)}


@pytest.mark.parametrize("nepochs", [1, 37])
@pytest.mark.parametrize("nbatch", [1, 3, 300])
@pytest.mark.parametrize("dname", ["f64", "f32"])
@pytest.mark.parametrize("grid", MAIN)
def test_members_equal_single_runs_shared_table(grid, dname, nbatch, nepochs):
    """One [E] table of step sizes for all members (member stride 0)."""
    ref = reference(grid, dname, nepochs, False)
    ens = ensemble_of(grid, dname, nbatch)
    losses, norms = run_ensemble(ens, [ref["table"][0]])
    assert_members_equal(ens, losses, norms, ref, (grid, dname, nbatch, nepochs))


@pytest.mark.parametrize("nbatch", [3, 300])
@pytest.mark.parametrize("dname", ["f64", "f32"])
@pytest.mark.parametrize("grid", MAIN)
def test_members_equal_single_runs_per_member_lrs(grid, dname, nbatch):
    """A [B, E] table: every member steps with its own lr, and equals the single run with that lr."""
    ref = reference(grid, dname, 37, True)
    ens = ensemble_of(grid, dname, nbatch)
    losses, norms = run_ensemble(ens, [ref["table"][:nbatch]])
    assert_members_equal(ens, losses, norms, ref, (grid, dname, nbatch))
    assert not torch.equal(ens.x[0], ens.x[1])


def test_global_memory_form_in_float32():
    """k_poisson_small_epochs_batch<float, false>: a grid whose float32 state exceeds the LDS (forced, 2-D)."""
    ref = reference("2d-64x96", "f32", 37, True)
    ens = ensemble_of("2d-64x96", "f32", 3)
    losses, norms = run_ensemble(ens, [ref["table"][:3]])
    assert_members_equal(ens, losses, norms, ref, "2d-64x96 f32")


@pytest.mark.parametrize("grid,dname", [("1d-256", "f64"), ("2d-16", "f32"), ("2d-40x94", "f64")])
def test_two_chunks_equal_one(grid, dname):
    """State and moments persist across launches: 5 + 32 epochs in two launches equal 37 in one (both tables)."""
    for per_member in (False, True):
        ref = reference(grid, dname, 37, per_member)
        ens = ensemble_of(grid, dname, 5)
        table = ref["table"][:5] if per_member else ref["table"][0]
        losses, norms = run_ensemble(ens, [table[..., :5], table[..., 5:]])
        assert_members_equal(ens, losses, norms, ref, (grid, dname, per_member))


@pytest.mark.parametrize("grid,dname", [("1d-256", "f64"), ("2d-40x94", "f64"), ("2d-12x94", "f32")])
def test_run_to_run_reproducible(grid, dname):
    ref = reference(grid, dname, 37, True)
    runs = []
    for _ in range(2):
        ens = ensemble_of(grid, dname, BMAX)
        runs.append((ens,) + run_ensemble(ens, [ref["table"]]))
    (a, la, na), (b, lb, nb) = runs
    for name in ("x", "m", "v", "g"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(la, lb) and torch.equal(na, nb)


def test_member_strides_wider_than_a_member_are_respected():
    """Rows wider than a member (ops.poisson_small_epochs_batch takes the row strides as member strides): the members equal
    their single runs and the padding between them is not touched."""
    from odil_amd import ops

    grid, dname, nb, nep, pad = "2d-16", "f64", 3, 37, 5
    ref = reference(grid, dname, nep, True)
    ens = ensemble_of(grid, dname, nb)
    wide = lambda t, fill: torch.cat([t, torch.full((nb, pad), fill, dtype=t.dtype, device=t.device)], dim=1)
    x, m, v, g, u = (wide(t, 777.0) for t in (ens.x, ens.m, ens.v, ens.g, ens.u))
    out = torch.full((2, nb, nep + pad), 777.0, dtype=ens.dtype, device=ens.device)
    table = wide(ref["table"][:nb], 777.0)
    partials = torch.full((nb, ens.partials.shape[1] + pad), 777.0, dtype=torch.float64, device=ens.device)
    ops.poisson_small_epochs_batch(x[:, :-pad], m[:, :-pad], v[:, :-pad], g[:, :-pad], u[:, :-pad], ens.fu, ens.rhs, ens.shapes,
                                   ens.h2, table[:, :nep], OMB1, OMB2, EPS, out[0][:, :nep], out[1][:, :nep], partials[:, :-pad])
    for t in (x, m, v, g, u, out[0], out[1], partials):
        assert bool((t[:, -pad:] == 777.0).all()), "padding between members was written"
    for name, t in dict(x=x, m=m, v=v, g=g, losses=out[0], norms=out[1]).items():
        assert torch.equal(t[:, :-pad], ref[name][:nb]), name


# ------------------------------------------------------------------------------------------- optimize_ensemble
def _api():
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    return odil, poisson


def _member(odil, poisson, b, epochs):
    """Member b of a sweep over examples/poisson 1-D N = 256: its own right-hand side and initial guess on every level."""
    args = poisson.parse_args(["--ndim", "1", "--N", "256"])
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
def test_optimize_ensemble_equals_optimize_grad(own_lrs, cadence, monkeypatch):
    """4 members of examples/poisson 1-D N = 256, 50 epochs: x, m, v of every member equal four `optimize_grad` runs
    exactly, the callbacks fire at the same epochs with equal losses and norms, and every member's state holds its result."""
    monkeypatch.setenv("ODIL_GRAPH", "0")
    odil, poisson = _api()
    nb, epochs = 4, 50
    lrs = [0.002, 0.005, 0.01, 0.02] if own_lrs else None

    def recorder(seen):
        def cb(state, epoch, pinfo):
            seen.append((epoch, float(np.array(pinfo["loss"])), float(np.array(pinfo["norms"][0]))))

        if cadence:
            cb.next_active = lambda epoch: (epoch // cadence + 1) * cadence
        return cb

    singles = []
    for b in range(nb):
        args, problem, state = _member(odil, poisson, b, epochs)
        args.lr = lrs[b] if own_lrs else LR
        seen = []
        arrays, info = odil.util.optimize_grad(args, "adam", problem, state, recorder(seen))
        assert problem._fused.__dict__.get("_small_u") is not None, "the single run did not take the whole-epoch route"
        singles.append((seen, [a.clone() for a in arrays], [a.clone() for a in info.m], [a.clone() for a in info.v]))

    built = [_member(odil, poisson, b, epochs) for b in range(nb)]
    args, problems, states = built[0][0], [p for _, p, _ in built], [s for _, _, s in built]
    seen = [[] for _ in range(nb)]
    per_member = [recorder(s) for s in seen]

    def callback(member, state, epoch, pinfo):
        assert state is states[member]
        per_member[member](state, epoch, pinfo)

    if cadence:
        callback.next_active = per_member[0].next_active
    arrays, info = odil.util.optimize_ensemble(args, problems, states, callback, lrs=lrs)
    assert len(arrays) == nb and info.epochs == epochs and tuple(info.losses.shape) == (nb, epochs)
    want_epochs = [0] + (list(range(cadence, epochs + 1, cadence)) if cadence else list(range(1, epochs + 1)))
    for b in range(nb):
        ref_seen, x, m, v = singles[b]
        assert [e for e, _, _ in ref_seen] == want_epochs
        assert seen[b] == ref_seen, ("callbacks of member", b)
        final = problems[b].domain.arrays_from_state(states[b])
        for name, got, want in (("x", arrays[b], x), ("m", info.m[b], m), ("v", info.v[b], v), ("state", final, x)):
            assert len(got) == len(want) == 8
            for lvl, (p, q) in enumerate(zip(got, want)):
                assert p.shape == q.shape and torch.equal(p, q), (b, name, lvl, float((p - q).abs().max()))
    assert not torch.equal(arrays[0][0], arrays[1][0])


def test_optimize_ensemble_without_callback_runs_one_launch(monkeypatch):
    """No callback: all epochs of all members in one launch, the same result as with one."""
    from odil_amd import ops

    odil, poisson = _api()
    launches = []
    batch = ops.poisson_small_epochs_batch
    monkeypatch.setattr(ops, "poisson_small_epochs_batch", lambda *a: (launches.append(tuple(a[13].shape)), batch(*a))[1])
    results = []
    for cb in (None, lambda member, state, epoch, pinfo: None):
        built = [_member(odil, poisson, b, 50) for b in range(3)]
        arrays, info = odil.util.optimize_ensemble(built[0][0], [p for _, p, _ in built], [s for _, _, s in built], cb)
        results.append([a.clone() for member in arrays for a in member] + [info.losses.clone()])
    assert launches == [(3, 50)] + [(3, 1)] * 50
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_optimize_ensemble_refuses_another_operator(monkeypatch):
    """A member whose operator is not the Poisson stencil (found by probing it on the device) is named; nothing runs."""
    odil, poisson = _api()
    monkeypatch.setattr(odil.runtime, "enable_trace", False)  # (no kernel is generated for the operator that is refused)
    built = [_member(odil, poisson, b, 5) for b in range(3)]
    problems, states = [p for _, p, _ in built], [s for _, _, s in built]
    domain = problems[2].domain
    problems[2] = odil.Problem(lambda ctx: [ctx.field("u") * 2 - ctx.extra.rhs], domain, problems[2].extra)
    before = [a.clone() for a in domain.arrays_from_state(states[0])]
    with pytest.raises(ValueError, match="member 2: the operator is not the recognised Poisson stencil"):
        odil.util.optimize_ensemble(built[0][0], problems, states)
    for a, b in zip(domain.arrays_from_state(states[0]), before):
        assert torch.equal(a, b)
