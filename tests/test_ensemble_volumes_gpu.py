"""The ensemble of 3-D Poisson problems as batched launches -- odil_poisson_residual_synth_batch,
odil_poisson_adjoint_adam_volumes, odil_mg_synth_adj_adam_members, odil_mg_synth on [B, *shape] arrays
(csrc/poisson_synth_tile.hip, csrc/poisson.hip, csrc/mg_transfer.hip, csrc/mg_march.hip, csrc/mg_fast.hip),
fused.PoissonVolumeEnsemble, AdamNativeOptimizer.run_ensemble, util.optimize_ensemble(form="volumes") -- against each
member's own loop of `PoissonEvaluator.loss_grad_arrays(adam=...)`: the launches a single `optimize_grad` run makes.

Member b of a batched launch runs the single kernel's per-thread arithmetic on its own arrays and its loss is summed in the
single launch's order, so the requirement is EXACT equality (torch.equal): x, m, v of every level, and every epoch's loss
and norm.  Right-hand sides and starts differ per member: a member that computed another's data could not pass.

Grids (the smallest that reach each code path; level shapes fine -> coarse):
  4          (4,4,4), (2,2,2)              the minimum; coarse extent 2: reflected halo rows
  8x12x20    (8,12,20) -> (2,3,5)          non-cubic, odd coarse extents, h^2 no power of two on two axes (division path)
  8x40x80    (8,40,80), (4,20,40)          3 x 2 residual tiles per member with ragged last tiles
  64x8x16    (64,8,16) -> (16,2,4)         several z-chunks per member (test_ensemble_volumes_host.py counts them)
  8x32x128   (8,32,128) -> (2,8,32), f64   the single run takes the one-pass adjoint + first transpose launch (the ensemble
                                           the separate kernels); level 1 reaches the LDS-tile transpose
  32         32^3 -> 4^3, 4 levels         the use case
  8x8x64     (8,8,64), (4,4,32)            float32: the row-marching transpose (fine rows of 64 cells), whose volume index is
                                           not a grid coordinate
  8x32x512   (8,32,512), (4,16,256), f32   float32 with the one-pass launch in the single run and the two-column LDS-tile
                                           transpose in the ensemble (at (8,32,128) the separate float32 transpose is the
                                           row-marching kernel, which rounds differently: volumes_refusal refuses that shape)
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
    "4": ((4, 4, 4), 2),
    "8x12x20": ((8, 12, 20), 3),
    "8x40x80": ((8, 40, 80), 2),
    "64x8x16": ((64, 8, 16), 3),
    "8x32x128": ((8, 32, 128), 3),
    "32": ((32, 32, 32), 4),
    "8x8x64": ((8, 8, 64), 2),
    "8x32x512": ((8, 32, 512), 2),
}
ONE_PASS = ("8x32x128", "8x32x512")
DTYPES = {"f64": torch.float64, "f32": torch.float32}
# (every grid in both precisions but the one-pass grid, which the issue sets in float64)
CASES = [(grid, dname) for grid in GRIDS for dname in DTYPES
         if (grid, dname) not in (("8x32x128", "f32"), ("8x32x512", "f64"))]


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
    gen = torch.Generator().manual_seed(17 + len(grid))
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
    `optimize_grad` runs it eagerly, with today's defaults (the one-pass adjoint + transpose launch where the shape
    takes it).  (x, m, v level lists, losses [E], norms [E])."""
    evs, x0 = inputs(grid, dname)
    omb1, omb2 = adam_constants(dname, native)
    ev = evs[member]
    assert ev.synth_residual and ev.fuse_transpose == (grid in ONE_PASS)
    x = [t[member].clone() for t in x0]
    m, v = [torch.zeros_like(t) for t in x], [torch.zeros_like(t) for t in x]
    losses, norms = [], []
    for alpha in step_sizes(DTYPES[dname], member_lr(member, per_member), nepochs):
        loss, _ = ev.loss_grad_arrays(x, adam=(m, v, alpha, omb1, omb2, EPS))
        losses.append(loss.clone())
        norms.append(torch.sqrt(loss))
    losses, norms = torch.stack(losses), torch.stack(norms)
    assert bool(torch.isfinite(x[0]).all()) and bool((losses > 0).all())
    return x, m, v, losses, norms


def ensemble_of(grid, dname, ids, pad=0):
    from odil_amd import fused

    evs, x0 = inputs(grid, dname)
    ens = fused.PoissonVolumeEnsemble([evs[k] for k in ids], pad=pad)
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


def test_float32_members_of_the_one_pass_shape_with_row_marching_transposes_are_refused():
    """(8,32,128) in float32: the single run's one-pass launch sums the first transpose in the tile kernel's order, the
    separate float32 transpose of that shape is the row-marching kernel: refused by name, nothing launched."""
    from odil_amd import fused

    evs, _ = inputs("8x32x128", "f32")
    with pytest.raises(ValueError, match="ensemble member 0: .*one-pass"):
        fused.PoissonVolumeEnsemble(evs[:3])


# ------------------------------------------------------------------------------------------------- kernel level
def _wide(nb, shape, k, dtype, values=None):
    """([nb, cells + k] base filled with 777, its [nb, *shape] view): k elements of padding after every member."""
    cells = int(np.prod(shape))
    base = torch.full((nb, cells + k), 777.0, dtype=dtype, device="cuda:0")
    view = base[:, :cells].unflatten(1, shape)
    if values is not None:
        view.copy_(values)
    return base, view


# pad 2 and 6 elements of float64; in float32 the same 16 and 48 bytes (2 and 6 floats are off the 16-byte grid, which
# the launchers refuse: asserted below)
PADS = {"f64": (2, 6), "f32": (4, 12)}


@pytest.mark.parametrize("which", [0, 1], ids=["pad-16B", "pad-48B"])
@pytest.mark.parametrize("per_member", [False, True], ids=["alpha", "alphas"])
@pytest.mark.parametrize("grid,dname", CASES)
def test_residual_and_adjoint_launches_equal_their_single_forms(grid, dname, per_member, which):
    """ops.poisson_residual_synth_batch against ops.poisson_residual_synth, and ops.poisson_adjoint_adam_volumes against
    ops.poisson_adjoint_adam, per member: fu, loss, g, x, m, v bit for bit, with shared and per-member step sizes, with
    EVERY member stride wider than a member, and nothing written between the members or behind a workspace row."""
    from odil_amd import _lib, ops

    dtype, nb, pad = DTYPES[dname], 3, PADS[dname][which]
    evs, x0 = inputs(grid, dname)
    shape, cshape = evs[0].cshape, evs[0].shapes[1]
    cells = evs[0].sizes[0]
    gen = torch.Generator().manual_seed(5)
    rnd = lambda s=shape: torch.randn((nb,) + tuple(s), generator=gen, dtype=torch.float64).to(dtype).to("cuda:0")
    coarse = rnd(cshape).contiguous()
    (wb, w0), (rb, rhs), (fb, fu) = _wide(nb, shape, pad, dtype, rnd()), _wide(nb, shape, pad, dtype, rnd()), _wide(nb, shape, pad, dtype)
    (gb, g), (xb, x), (mb, m), (vb, v) = (_wide(nb, shape, pad, dtype), _wide(nb, shape, pad, dtype, rnd()),
                                          _wide(nb, shape, pad, dtype, 0.1 * rnd()), _wide(nb, shape, pad, dtype, rnd().abs()))
    x_in, m_in, v_in = x.clone(), m.clone(), v.clone()
    nsums, npart = ops.residual_synth_batch_workspace(cshape)
    partials = torch.full((nb, npart + 3), 777.0, dtype=torch.float64, device="cuda:0")
    sums = torch.full((nb + 1, nsums), 777.0, dtype=torch.float64, device="cuda:0")
    loss = torch.zeros(nb, dtype=dtype, device="cuda:0")
    alphas = torch.tensor([0.001, 0.002, 0.003] if per_member else [0.002], dtype=dtype, device="cuda:0")
    h2, scale = evs[0].h2, float(evs[0].scale)
    ops.poisson_residual_synth_batch(coarse, w0, rhs, h2, fu, loss, partials[:, :npart], sums[:nb])
    ops.poisson_adjoint_adam_volumes(fu, h2, scale, g, x, m, v, alphas, OMB1, OMB2, EPS)
    for b in range(nb):
        fu1, loss1 = ops.poisson_residual_synth(coarse[b], w0[b].contiguous(), rhs[b].contiguous(), h2)
        x1, m1, v1 = x_in[b].clone(), m_in[b].clone(), v_in[b].clone()
        alpha = float(alphas[b if per_member else 0])
        g1 = ops.poisson_adjoint_adam(fu1, h2, scale, torch.empty_like(fu1), x1, m1, v1, alpha, OMB1, OMB2, EPS)
        for name, got, want in (("fu", fu[b], fu1), ("loss", loss[b], loss1), ("g", g[b], g1), ("x", x[b], x1),
                                ("m", m[b], m1), ("v", v[b], v1)):
            assert torch.equal(got, want), (grid, dname, b, name)
    for k, base in enumerate((wb, rb, fb, gb, xb, mb, vb)):
        assert bool((base[:, cells:] == 777.0).all()), ("padding written", k)
    assert bool((partials[:, npart:] == 777.0).all()) and bool((sums[nb] == 777.0).all())
    # the gradient not stored: the same update
    x2, m2, v2 = x_in.clone(), m_in.clone(), v_in.clone()
    ops.poisson_adjoint_adam_volumes(fu, h2, scale, None, x2, m2, v2, alphas, OMB1, OMB2, EPS)
    assert torch.equal(x2, x) and torch.equal(m2, m) and torch.equal(v2, v)
    if dname == "f32":  # 2 floats between the members: off the 16-byte grid
        _, bad = _wide(nb, shape, 2, dtype)
        with pytest.raises(_lib.OdilHipError, match="not a multiple of 16 bytes"):
            ops.poisson_residual_synth_batch(coarse, w0, rhs, h2, bad, loss, partials[:, :npart], sums[:nb])


@pytest.mark.parametrize("per_member", [False, True], ids=["alpha", "alphas"])
@pytest.mark.parametrize("grid,dname", CASES)
def test_transpose_chain_equals_its_single_form(grid, dname, per_member):
    """ops.mg_synth_adj_adam_members on 'ccc' rows against ops.mg_synth_adj_adam on each member alone: the gradients and x, m, v of the
    levels 1 ... equal bit for bit (every level runs the kernel a single volume's level runs, and that kernel reads the
    member's step size); and the coarse synthesis on [B, *shape] arrays equals the single volumes'."""
    from odil_amd import ops

    dtype, nb = DTYPES[dname], 3
    evs, x0 = inputs(grid, dname)
    shapes = evs[0].shapes
    gen = torch.Generator().manual_seed(9)
    rnd = lambda s: torch.randn((nb,) + tuple(s), generator=gen, dtype=torch.float64).to(dtype).to("cuda:0")
    gu = rnd(shapes[0])
    x, m, v = [rnd(s) for s in shapes], [0.1 * rnd(s) for s in shapes], [rnd(s).abs() for s in shapes]
    x_in, m_in, v_in = [t.clone() for t in x], [t.clone() for t in m], [t.clone() for t in v]
    grads = [gu] + [torch.full((nb,) + s, 777.0, dtype=dtype, device="cuda:0") for s in shapes[1:]]
    alphas = torch.tensor([0.001, 0.002, 0.003] if per_member else [0.002], dtype=dtype, device="cuda:0")
    ops.mg_synth_adj_adam_members(gu, shapes, "ccc", grads, x, m, v, alphas, OMB1, OMB2, EPS)
    for b in range(nb):
        x1, m1, v1 = [t[b].clone() for t in x_in], [t[b].clone() for t in m_in], [t[b].clone() for t in v_in]
        g1 = [gu[b].clone()] + [torch.empty(s, dtype=dtype, device="cuda:0") for s in shapes[1:]]
        alpha = float(alphas[b if per_member else 0])
        ops.mg_synth_adj_adam(g1[0], shapes, "ccc", g1, x1, m1, v1, alpha, OMB1, OMB2, EPS)
        for lvl in range(1, len(shapes)):
            for name, got, want in (("g", grads, g1), ("x", x, x1), ("m", m, m1), ("v", v, v1)):
                assert torch.equal(got[lvl][b], want[lvl]), (grid, dname, b, name, lvl)
        assert torch.equal(x[0][b], x_in[0][b])  # (level 0 belongs to the stencil adjoint)
    if len(shapes) > 2:
        coarse = ops.mg_synth(x_in[1:], ".ccc")
        for b in range(nb):
            assert torch.equal(coarse[b], ops.mg_synth([t[b].contiguous() for t in x_in[1:]], "ccc")), (grid, dname, b)


# ------------------------------------------------------------------------------------------------------- epochs
@pytest.mark.parametrize("per_member", [False, True], ids=["lr", "lrs"])
@pytest.mark.parametrize("nepochs", [5, 12])
@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("grid,dname", CASES)
def test_members_equal_single_runs(grid, dname, nbatch, nepochs, per_member):
    ids = list(range(nbatch))
    ens = ensemble_of(grid, dname, ids)
    losses, norms = run_epochs(ens, [table_of(dname, ids, nepochs, per_member)])
    assert_members_equal(ens, losses, norms, grid, dname, ids, nepochs, per_member)
    if per_member and nbatch > 1:
        assert not torch.equal(ens.x[-1][0], ens.x[-1][1])


@pytest.mark.parametrize("nepochs,per_member", [(5, False), (12, True)], ids=["5-lr", "12-lrs"])
@pytest.mark.parametrize("grid,dname", CASES)
def test_seventy_members_and_the_position_of_a_member(grid, dname, nepochs, per_member):
    """B = 70, and a member's result does not depend on where it stands: member 0 at position 41 of 70 and at position
    0 of 3 both equal its single run."""
    ids = list(range(1, 42)) + [0] + list(range(42, BMAX))
    assert len(ids) == BMAX and ids[41] == 0
    ens = ensemble_of(grid, dname, ids)
    losses, norms = run_epochs(ens, [table_of(dname, ids, nepochs, per_member)])
    assert_members_equal(ens, losses, norms, grid, dname, ids, nepochs, per_member)
    few = ensemble_of(grid, dname, [0, 1, 2])
    few_losses, _ = run_epochs(few, [table_of(dname, [0, 1, 2], nepochs, per_member)])
    assert torch.equal(few_losses[0], losses[41])
    for a, b in zip(few.levels(few.x, 0), ens.levels(ens.x, 41)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("grid,dname,pad", [("8x12x20", "f64", 2), ("64x8x16", "f64", 6), ("8x40x80", "f32", 4),
                                            ("32", "f32", 12)])
def test_member_strides_wider_than_a_member(grid, dname, pad):
    """fu, rhs, m[0], v[0] of the ensemble with `pad` elements (a multiple of 16 bytes) between the members: the members
    equal their single runs and the padding is not written."""
    ids = [0, 1, 2]
    ens = ensemble_of(grid, dname, ids, pad=pad)
    cells = ens.cells
    assert ens.fu.stride(0) == cells + pad == ens.m[0].stride(0) == ens.v[0].stride(0) == ens.rhs.stride(0)
    losses, norms = run_epochs(ens, [table_of(dname, ids, 5, True)])
    assert_members_equal(ens, losses, norms, grid, dname, ids, 5, True)
    for t in (ens.fu, ens.m[0], ens.v[0], ens.rhs):
        rows = t.as_strided((3, cells + pad), (cells + pad, 1))
        assert bool((rows[:, cells:] == 0).all()), "padding between members was written"


@pytest.mark.parametrize("grid,dname", CASES)
def test_two_chunks_equal_one(grid, dname):
    """State and moments persist across calls: 5 + 7 epochs in two calls equal 12 in one (both kinds of table)."""
    ids = [0, 1, 2]
    for per_member in (False, True):
        ens = ensemble_of(grid, dname, ids)
        table = table_of(dname, ids, 12, per_member)
        losses, norms = run_epochs(ens, [table[..., :5], table[..., 5:]])
        assert_members_equal(ens, losses, norms, grid, dname, ids, 12, per_member)


@pytest.mark.parametrize("grid,dname", [("64x8x16", "f64"), ("8x32x128", "f64"), ("32", "f32")])
def test_run_to_run_reproducible(grid, dname):
    ids = list(range(BMAX))
    runs = []
    for _ in range(2):
        ens = ensemble_of(grid, dname, ids)
        runs.append((ens,) + run_epochs(ens, [table_of(dname, ids, 5, True)]))
    (a, la, na), (b, lb, nb) = runs
    for name in ("x", "m", "v", "g"):
        for p, q in zip(getattr(a, name), getattr(b, name)):
            assert torch.equal(p, q), name
    assert torch.equal(la, lb) and torch.equal(na, nb)


@pytest.mark.parametrize("per_member", [False, True], ids=["lr", "lrs"])
@pytest.mark.parametrize("grid,dname", [("8x12x20", "f64"), ("8x32x128", "f64"), ("32", "f32")])
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
@pytest.mark.parametrize("form,own_lrs", [("volumes", False), ("volumes", True), ("auto", True)])
def test_optimize_ensemble_volumes_equals_optimize_grad(form, own_lrs, cadence, monkeypatch):
    """4 members of examples/poisson --ndim 3 --N 16, 30 epochs, form="volumes" / "auto": x, m, v of every member equal
    four `optimize_grad` runs exactly, the callbacks fire at the same epochs with equal losses and norms, and every
    member's state holds its result.  form="launches" and the default form keep refusing these members."""
    monkeypatch.setenv("ODIL_GRAPH", "0")
    odil, poisson = _api()
    spec, nb, epochs = "--ndim 3 --N 16", 4, 30
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
    with pytest.raises(ValueError, match="member 0: 3-D grid: the batched launches run 1-D and 2-D grids"):
        odil.util.optimize_ensemble(args, problems, states, form="launches")
    with pytest.raises(ValueError, match="member 0: 3-D grid: the one-workgroup epochs run 1-D and 2-D grids"):
        odil.util.optimize_ensemble(args, problems, states)
    seen = [[] for _ in range(nb)]
    per_member = [recorder(s) for s in seen]

    def callback(member, state, epoch, pinfo):
        assert state is states[member]
        per_member[member](state, epoch, pinfo)

    if cadence:
        callback.next_active = per_member[0].next_active
    arrays, info = odil.util.optimize_ensemble(args, problems, states, callback, lrs=lrs, form=form)
    assert type(info.ensemble).__name__ == "PoissonVolumeEnsemble"
    assert len(arrays) == nb and info.epochs == epochs and tuple(info.losses.shape) == (nb, epochs)
    want_epochs = [0] + (list(range(cadence, epochs + 1, cadence)) if cadence else list(range(1, epochs + 1)))
    for b in range(nb):
        ref_seen, x, m, v = singles[b]
        ref_at = {e: (l, n) for e, l, n in ref_seen}
        assert [e for e, _, _ in seen[b]] == want_epochs
        assert seen[b] == [(e,) + ref_at[e] for e in want_epochs], ("callbacks of member", b)
        final = problems[b].domain.arrays_from_state(states[b])
        for name, got, want in (("x", arrays[b], x), ("m", info.m[b], m), ("v", info.v[b], v), ("state", final, x)):
            assert len(got) == len(want) >= 2
            for lvl, (p, q) in enumerate(zip(got, want)):
                assert p.shape == q.shape and torch.equal(p, q), (b, name, lvl, float((p - q).abs().max()))
    assert not torch.equal(arrays[0][0], arrays[1][0])


def test_optimize_ensemble_volumes_without_callback_and_another_operator(monkeypatch):
    """No callback: the same result as the single runs; an operator that is not the Poisson stencil is refused by name."""
    odil, poisson = _api()
    spec, nb, epochs = "--ndim 3 --N 16", 3, 12
    singles = []
    for b in range(nb):
        args, problem, state = _member(odil, poisson, spec, b, epochs)
        arrays, info = odil.util.optimize_grad(args, "adam", problem, state, None)
        singles.append([a.clone() for a in arrays])
    built = [_member(odil, poisson, spec, b, epochs) for b in range(nb)]
    args, problems, states = built[0][0], [p for _, p, _ in built], [s for _, _, s in built]
    arrays, info = odil.util.optimize_ensemble(args, problems, states, form="volumes")
    for b in range(nb):
        for p, q in zip(arrays[b], singles[b]):
            assert torch.equal(p, q), b

    built = [_member(odil, poisson, spec, b, epochs) for b in range(2)]
    args, problems, states = built[0][0], [p for _, p, _ in built], [s for _, _, s in built]
    monkeypatch.setattr(odil.runtime, "enable_trace", False)  # (no kernel is generated for the operator that is refused)
    problems[1] = odil.Problem(lambda ctx: [ctx.field("u") * 2 - ctx.extra.rhs], problems[1].domain, problems[1].extra)
    with pytest.raises(ValueError, match="member 1: the operator is not the recognised Poisson stencil"):
        odil.util.optimize_ensemble(args, problems, states, form="volumes")
