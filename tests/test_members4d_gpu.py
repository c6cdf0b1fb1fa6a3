"""Ensembles of 4-D members on the device: the transfers on the R rows of [R, t, x, y, z] level arrays
(`ops.mg_synth_adj_adam_members` with ndim 4, `ops.mg_synth_members`) against the single calls on every row alone, and
`odil.util.optimize_ensemble` for members on (t, x, y, z) (`fused.TracedLaunchEnsemble`: examples/velocity_from_tracer/
veltracer3d.py, four fields at 'nccc'; one 'cccc' unknown; an `Array` behind it) against every member's own `optimize_grad`
run -- bit for bit (`torch.equal`), with Adam and with L-BFGS-B, in float64 and in float32.  Members and layouts:
tests/members4d.py; every test of a run asserts that every field left its start on its finest and its coarsest level."""

import os

import numpy as np
import pytest
import torch
from fields_ensemble_members import run_args
from members4d import FAST, GENERIC, LAYOUT_IDS, LAYOUTS4, NODE, TRACER3D_LEVELS, cell4, kinds_of, net4, tracer3d
from test_fields_ensemble_gpu import CANARY, LRS, fields_moved, guarded
from test_param_ensemble_gpu import single_runs as single_runs_any
from test_traced_ensemble_gpu import assert_equal_single, ensemble_run, numbers, single_runs

import odil_amd as odil
from odil_amd import _lib, ops, stencil_bind
from odil_amd.core import Array

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")]
TDTYPES = [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")]


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    saved = odil.util.g_log_file
    odil.util.set_log_file(open(os.devnull, "w"))
    monkeypatch.setenv("ODIL_GRAPH", "0")  # (six epochs never replay; the test of the replay sets it itself)
    yield
    odil.util.g_log_file = saved


def canaries_intact(pairs):
    return all(bool((buf[:8] == CANARY).all()) and bool((buf[-8:] == CANARY).all()) for _, buf in pairs)


# ------------------------------------------------------------------------ (a) ops.mg_synth_adj_adam_members on 4-D rows
@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("loc,shapes,kinds", LAYOUTS4, ids=LAYOUT_IDS)
def test_members_chain_equals_the_single_chain_and_adam_step_per_row(loc, shapes, kinds, dtype):
    """The pattern of tests/test_fields_ensemble_gpu.py on rows of four axes: six rows, step sizes of period three,
    canaries of 64 bytes on either side of every level array."""
    nrows, period = 6, 3
    lib = _lib.load()
    esize = 8 if dtype == torch.float64 else 4
    # the transposes a single row runs: a change of the selection rules must not quietly empty this test
    assert kinds_of(lib, _lib.i64, loc, shapes, esize) == kinds and set(kinds) <= {GENERIC, FAST, NODE}
    gen = torch.Generator().manual_seed(11 + len(shapes))
    draw = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)
    gu = draw(nrows, *shapes[0]).cuda()
    alphas = torch.tensor([0.01, 0.02, 0.005], dtype=dtype).cuda()
    omb1, omb2, eps = 1 - np.float64(0.9), 1 - np.float64(0.999), 1e-7
    x, m, v, g = ([None] + [guarded(fill(nrows, *s)) for s in shapes[1:]]
                  for fill in (draw, draw, lambda *s: draw(*s).abs(), lambda *s: torch.full(s, 7.0, dtype=dtype)))
    tensors = lambda lst: [None] + [t for t, _ in lst[1:]]
    start, start_m, start_v = ([t.clone() for t in tensors(lst)[1:]] for lst in (x, m, v))
    # per row: the single chain on that row alone, then the plain update of every level >= 1
    want = []
    for r in range(nrows):
        grads = ops.mg_synth_adj(gu[r].clone(), shapes, loc)
        rows = []
        for l in range(1, len(shapes)):
            xs, ms, vs = (lst[l][0][r].clone() for lst in (x, m, v))
            ops.adam_step(xs.view(-1), ms.view(-1), vs.view(-1), grads[l].reshape(-1), alphas[r % period:][:1], omb1, omb2, eps)
            rows.append((grads[l], xs, ms, vs))
        want.append(rows)
    flat = [int(n) for s in shapes for n in s]
    assert lib.odil_mg_members_levels_ok(_lib.i64(flat), len(shapes), 4, loc.encode(), nrows, esize) == 0
    assert lib.odil_mg_members_levels_ok(_lib.i64(flat), len(shapes), 4, loc.encode(), 70000, esize) != 0
    assert "70000 rows" in lib.odil_last_error().decode()
    # the gradients alone: x, m, v untouched
    before = [buf.clone() for lst in (x, m, v) for _, buf in lst[1:]]
    ops.mg_synth_adj_adam_members(gu, shapes, loc, tensors(g))
    for r in range(nrows):
        for l in range(1, len(shapes)):
            assert torch.equal(g[l][0][r], want[r][l - 1][0]), (r, l, float((g[l][0][r] - want[r][l - 1][0]).abs().max()))
    assert all(torch.equal(buf, old) for (_, buf), old in zip([p for lst in (x, m, v) for p in lst[1:]], before))
    for t, _ in g[1:]:
        t.fill_(7.0)
    # with the update: row r with alphas[r % period]
    ops.mg_synth_adj_adam_members(gu, shapes, loc, tensors(g), tensors(x), tensors(m), tensors(v), alphas, omb1, omb2, eps,
                                  period=period)
    for r in range(nrows):
        for l in range(1, len(shapes)):
            for name, got, ref in zip("gxmv", (g[l][0][r], x[l][0][r], m[l][0][r], v[l][0][r]), want[r][l - 1]):
                assert torch.equal(got, ref), (name, r, l, float((got - ref).abs().max()))
    assert all(not torch.equal(now, old) for now, old in zip(tensors(x)[1:], start))
    assert not torch.equal(x[1][0][0] - start[0][0], x[1][0][1] - start[0][1])
    for lst in (x, m, v, g):  # the canaries before and behind every level array
        assert canaries_intact(lst[1:])

    # a step size per row (period 0) gives what the period gives; one element is shared by all rows
    def run(steps, period):
        xs, ms, vs = ([None] + [t.clone() for t in part] for part in (start, start_m, start_v))
        gs = [None] + [torch.empty_like(t) for t in start]
        ops.mg_synth_adj_adam_members(gu, shapes, loc, gs, xs, ms, vs, steps, omb1, omb2, eps, period=period)
        return xs[1:] + ms[1:] + vs[1:] + gs[1:]

    per_row, by_period = run(alphas.repeat(nrows // period), 0), run(alphas, period)
    assert all(torch.equal(p, q) for p, q in zip(per_row, by_period))
    assert all(torch.equal(p, q) for p, q in zip(by_period[:len(start)], tensors(x)[1:]))
    shared, spelled = run(alphas[1:2].clone(), 0), run(alphas[1:2].repeat(nrows), 0)
    assert all(torch.equal(p, q) for p, q in zip(shared, spelled))


# ------------------------------------------------------------------------------------------- (b) ops.mg_synth_members
SYNTH_LAYOUTS = [(loc, shapes) for loc, shapes, _ in LAYOUTS4] + [("ncc", [(5, 8, 16), (3, 4, 8)]), ("nc", [(9, 16), (5, 8), (3, 4)])]


@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("nrows", [1, 6])
@pytest.mark.parametrize("loc,shapes", SYNTH_LAYOUTS, ids=["{}-{}".format(l, "x".join(map(str, s[0]))) for l, s in SYNTH_LAYOUTS])
def test_row_synthesis_equals_the_single_synthesis(loc, shapes, nrows, dtype):
    gen = torch.Generator().manual_seed(17 + nrows)
    draw = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)
    terms = [guarded(draw(nrows, *s)) for s in shapes]
    kept = [buf.clone() for _, buf in terms]
    want = [ops.mg_synth([t[r].clone() for t, _ in terms], loc) for r in range(nrows)]
    # work not given
    out = guarded(torch.full((nrows,) + shapes[0], 7.0, dtype=dtype))
    res = ops.mg_synth_members([t for t, _ in terms], loc, out=out[0])
    assert res is out[0]
    for r in range(nrows):
        assert torch.equal(out[0][r], want[r]), (r, float((out[0][r] - want[r]).abs().max()))
    # work given
    work = [None] + [guarded(torch.full((nrows,) + s, 7.0, dtype=dtype)) for s in shapes[1:-1]] + [None]
    out2 = guarded(torch.full((nrows,) + shapes[0], 7.0, dtype=dtype))
    ops.mg_synth_members([t for t, _ in terms], loc, work=[None if w is None else w[0] for w in work], out=out2[0])
    assert torch.equal(out2[0], out[0])
    assert canaries_intact(terms + [out, out2] + [w for w in work if w is not None])
    assert all(torch.equal(buf, old) for (_, buf), old in zip(terms, kept))  # (the level arrays are read, never written)
    # without `out`: a new tensor
    assert torch.equal(ops.mg_synth_members([t for t, _ in terms], loc), out[0])
    if nrows > 1:
        assert not torch.equal(out[0][0], out[0][1])


# --------------------------------------------------------------------------------------- (c) the ensemble against single runs
# name -> (build(b, dtype), grid fields, arrays of a member)
CASES = dict([
    ("tracer3d-3lvl", (lambda b, dt: tracer3d(3, dt, b), 4, 12)),
    ("tracer3d-plain", (lambda b, dt: tracer3d(None, dt, b), 4, 4)),
    ("cell4-3lvl", (lambda b, dt: cell4(3, dt, b), 1, 3)),  # ONE 'cccc' unknown: the stacked rows all the same
    ("cell4-array", (lambda b, dt: cell4(2, dt, b, with_array=True), 1, 3)),  # an `Array` after the field
])
RUNS = [("tracer3d-3lvl", 1, False), ("tracer3d-3lvl", 3, True), ("tracer3d-3lvl", 5, False), ("tracer3d-plain", 1, True),
        ("tracer3d-plain", 3, False), ("tracer3d-plain", 5, True), ("cell4-3lvl", 3, True), ("cell4-array", 3, False)]


def level_kinds(ens):
    esize = 8 if ens.dtype == torch.float64 else 4
    return kinds_of(_lib.load(), _lib.i64, ens.loc[1:], ens.shapes, esize)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,nb,own_lrs", RUNS, ids=["{}-B{}-{}".format(c, n, "lrs" if o else "lr") for c, n, o in RUNS])
def test_adam_members_equal_their_single_runs(case, nb, own_lrs, dtype):
    """Six Adam epochs: x of every field and level (and `Array`), m, v, and every epoch's loss, terms, norms and names equal
    the members' own `optimize_grad` runs."""
    make, nfields, narrays = CASES[case]
    build = lambda b: make(b, dtype)
    args = run_args(epochs=6)
    lrs = LRS[:nb] if own_lrs else None
    singles = single_runs(build, nb, args, lrs)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "volumes" if nb != 3 else "auto", lrs)
    assert info.form == "volumes" and len(arrays[0]) == narrays
    assert_equal_single(arrays, info, seen, problems, states, singles)
    fields_moved(build, problems, states, nfields)
    ens = info.ensemble
    assert ens.ndim == 4 and ens.stacked and ens.nfields == nfields and ens.nrows == nfields * nb
    assert len(ens.batches) == 1 and ens.batches[0].uploads == 1
    assert ens.total == nfields * sum(ens.sizes) + ens.nparams == sum(a.numel() for a in arrays[0])
    assert tuple(ens.x[0].shape) == (nfields * nb,) + ens.cshape and ens.loc == "." + next(
        f.loc for f in states[0].fields.values() if not isinstance(f, Array))
    if case == "tracer3d-3lvl":  # (a node-centred marching level and a fast one: the levels the `Domain` plans)
        assert ens.shapes == TRACER3D_LEVELS and level_kinds(ens) == [NODE, FAST]
    elif case == "cell4-3lvl":
        assert ens.shapes == [(8,) * 4, (4,) * 4, (2,) * 4] and level_kinds(ens) == [FAST, FAST]


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_regularisation_weights_run_as_two_groups(dtype):
    """`kxreg` is a Python number of the operator: two values generate two sources, two groups of members -- and still ONE
    transposed chain and ONE level-0 update for all fields of all members."""
    nb, kx = 4, [0.01, 0.02, 0.01, 0.02]
    build = lambda b: tracer3d(2, dtype, b, cells=(4, 8, 8, 8), kxreg=kx[b])
    args = run_args(epochs=6)
    singles = single_runs(build, nb, args, LRS[:nb])
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "volumes", LRS[:nb])
    assert info.ensemble.groups == [[0, 2], [1, 3]]
    assert info.ensemble.shapes == [(5, 8, 8, 8), (3, 4, 4, 4)] and level_kinds(info.ensemble) == [NODE]
    assert_equal_single(arrays, info, seen, problems, states, singles)
    fields_moved(build, problems, states, 4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["tracer3d-3lvl", "cell4-3lvl"])
def test_lbfgsb_members_equal_their_single_runs(case, dtype):
    """Eight iterations in lock-step, bfgs_m = 5: every member ends where its own `lbfgsb` run ends."""
    make, nfields, narrays = CASES[case]
    build = lambda b: make(b, dtype)
    nb, args = 3, run_args("lbfgsb", epochs=8, bfgs_m=5)
    singles = single_runs_any(build, nb, args)
    problems, states, seen = [], [], [[] for _ in range(nb)]
    for b in range(nb):
        problem, state = build(b)
        problems.append(problem)
        states.append(state)
    callback = lambda member, state, epoch, pinfo: seen[member].append((epoch,) + numbers(pinfo))
    arrays, info = odil.util.optimize_ensemble(args, problems, states, callback, form="volumes")
    assert info.route == "traced" and info.form == "volumes" and info.ensemble.stacked
    assert all(int(n) >= 4 for n in info.nits), info.nits
    for b, (ref_seen, x, _, _, single) in enumerate(singles):
        assert int(info.nits[b]) == int(single.epochs) and int(info.evals[b]) == int(single.evals)
        assert seen[b] == ref_seen, ("reports of member", b)
        final = problems[b].domain.arrays_from_state(states[b])
        for got in (arrays[b], final):
            assert len(got) == len(x) == narrays
            for k, (p, q) in enumerate(zip(got, x)):
                assert p.shape == q.shape and torch.equal(p, q), (b, k, float((p - q).abs().max()))
    fields_moved(build, problems, states, nfields)


def test_a_4d_member_whose_forward_kernel_marches_is_refused_by_name():
    """`net4` in float32 with a last axis of 128 cells: ValueError naming the member (all members share the shape: the
    first is named), every state left as it was."""
    built = [net4(np.float32, b) for b in range(2)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    before = [[(a, a.clone()) for a in p.domain.arrays_from_state(s)] for p, s in built]
    with pytest.raises(ValueError, match="member 0: its operator has no batched kernels .*marching forward kernel"):
        odil.util.optimize_ensemble(run_args(), problems, states, form="volumes")
    for (p, s), old in zip(built, before):
        now = p.domain.arrays_from_state(s)
        assert len(now) == len(old) and all(a is b and torch.equal(a, copy) for a, (b, copy) in zip(now, old))


# ------------------------------------------------------------------------------------------------- (d) reference anchor
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_member_from_the_fixture_follows_the_reference(tag):
    """B = 3, member 0 built from the fixture as the single-run test builds it, the others perturbed: ten free epochs from
    the reference's state at epoch 1 against its state at epoch 11 and its loss of every epoch -- the single run's own
    bars (tests/test_traj_workloads_gpu.py `check_state`, tests/test_net_ensemble_gpu.py `LOSS_RTOL`)."""
    from conftest import load_golden
    from test_net_ensemble_gpu import LOSS_RTOL
    from test_traj_workloads_gpu import build, check_state, state_at

    t = load_golden("traj_adam_states_veltracer3d_{}".format(tag))
    lr = float(t["lr"])
    mod = odil.runtime.get_mod()
    problems, states = [], []
    for b in range(3):
        problem, state, n = build("veltracer3d", tag)
        x = [mod.array(a) for a in state_at(t, 1, n)[0]]
        if b:
            gen = torch.Generator().manual_seed(b)
            x = [a + 0.05 * torch.randn(a.shape, generator=gen, dtype=torch.float64).to(a.dtype).to(a.device) for a in x]
        problem.domain.arrays_to_state(x, state)
        problems.append(problem)
        states.append(state)

    def callback(member, state, epoch, pinfo):
        problems[member].tracers["epoch"] = epoch + 1

    arrays, info = odil.util.optimize_ensemble(run_args(epochs=10, lr=lr), problems, states, callback, form="volumes")
    assert info.route == "traced" and len(arrays[0]) == n and info.ensemble.nfields == 4 and info.ensemble.ndim == 4
    check_state((arrays[0], info.m[0], info.v[0]), state_at(t, 11, n), tag, lr, "free")
    losses = info.losses[0].cpu().numpy()
    for k in range(10):
        ref = float(t["losses"][k])
        print("epoch", k + 1, "loss", float(losses[k]), "reference", ref)
        assert abs(float(losses[k]) - ref) <= LOSS_RTOL[tag] * abs(ref), (k, float(losses[k]), ref)
    assert not torch.equal(arrays[0][0], arrays[1][0])


# ------------------------------------------------------------------------------------------------------ (e) launch count
def test_an_epoch_makes_the_same_launches_for_two_and_for_five_members(monkeypatch):
    """The library calls and generated launches of an epoch of `tracer3d` do not grow with B; the synthesis, the transposed
    chain and the level-0 update are called once per epoch for all four fields, the argument blocks are staged once."""
    called, launched = [], []
    real, real_launch = _lib.call, stencil_bind.EpochBatch.launch

    def counting(name, *args, **kwargs):
        called.append(name)
        return real(name, *args, **kwargs)

    def launching(self):
        launched.append(self.nb)
        return real_launch(self)

    monkeypatch.setattr(ops, "call", counting)
    monkeypatch.setattr(stencil_bind.EpochBatch, "launch", launching)
    per_epoch = dict()
    for nb in (2, 5):
        built = [tracer3d(3, np.float64, b) for b in range(nb)]
        _, info = odil.util.optimize_ensemble(run_args(epochs=0), [p for p, _ in built], [s for _, s in built], form="volumes")
        ens = info.ensemble
        alphas = torch.full((ens.nrows,), 0.01, dtype=ens.dtype, device=ens.device)
        del called[:], launched[:]
        for _ in range(3):
            ens.epoch(alphas, 0.1, 0.001, 1e-7)
        torch.cuda.synchronize()
        assert launched == [nb] * 3 and ens.batches[0].uploads == 1 and len(ens.batches) == 1
        per_epoch[nb] = list(called)
    assert per_epoch[2] == per_epoch[5]
    assert per_epoch[2] == ["mg_synth_members", "mg_synth_adj_adam_members", "adam_step_batch"] * 3


# ------------------------------------------------------------------------------------------------------ (e) graph replay
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["tracer3d-3lvl", "cell4-3lvl"])
def test_replayed_epochs_equal_eager_epochs(case, dtype, monkeypatch):
    make, nfields, narrays = CASES[case]
    build = lambda b: make(b, dtype)
    nb, args = 3, run_args(epochs=9)
    runs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("ODIL_GRAPH", mode)
        runs.append(ensemble_run(build, nb, args, "volumes", lrs=LRS[:nb]))
    (xa, ia, sa, _, _), (xb, ib, sb, pb, stb) = runs
    assert ia.ensemble.graphable and ib.ensemble.batches[0].uploads == 1
    assert torch.equal(ia.losses, ib.losses) and torch.equal(ia.norms, ib.norms) and sa == sb
    for b in range(nb):
        for got, want in ((xa[b], xb[b]), (ia.m[b], ib.m[b]), (ia.v[b], ib.v[b])):
            assert len(got) == narrays and all(torch.equal(p, q) for p, q in zip(got, want))
    fields_moved(build, pb, stb, nfields)
