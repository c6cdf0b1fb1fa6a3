"""Ensembles of inverse problems on the device: `odil.util.optimize_ensemble` for members with `Array` unknowns beside their
field (`fused.TracedLaunchEnsemble` with packed parameters, `stencil_bind.EpochBatch`, `ops.adam_step_params_batch`).
Every member, its constants included, must end where its own `optimize_grad` run ends, bit for bit (`torch.equal`), with
Adam and with L-BFGS-B, in float64 and in float32.  Members: tests/param_ensemble_members.py -- every one starts with its
constants at half their true values, and every test of a run asserts that the constants moved."""

import argparse
import os

import numpy as np
import pytest
import torch
from param_ensemble_members import TRUE, forward_only, make_member, run_args
from test_traced_ensemble_gpu import assert_equal_single, numbers

import odil_amd as odil
from odil_amd import ops, runtime
from odil_amd.optimizer import EarlyStopError

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")]
# (cells, levels of the MultigridField or None for a plain Field, form)
SHAPES = dict([
    ("1d-64-3lvl", ((64,), 3, "launches")),
    ("2d-16x24-3lvl", ((16, 24), 3, "launches")),
    ("2d-12x18-plain-field", ((12, 18), None, "launches")),
    ("3d-8x8x16-2lvl", ((8, 8, 16), 2, "volumes")),
])
# (shape, members, a step size per member, order of the state, the second Array)
RUNS = [("1d-64-3lvl", 3, False, "after", False), ("2d-16x24-3lvl", 1, False, "after", False),
        ("2d-16x24-3lvl", 3, False, "before", False), ("2d-16x24-3lvl", 5, True, "around", True),
        ("2d-12x18-plain-field", 3, False, "before", True), ("2d-12x18-plain-field", 5, True, "after", False),
        ("3d-8x8x16-2lvl", 3, False, "after", True), ("3d-8x8x16-2lvl", 1, False, "before", False),
        ("3d-8x8x16-2lvl", 5, True, "around", True)]


def coeff_shape(shape, order):
    """(3,); four elements (the last never read) where `coeff` alone stands before a 3-D multigrid field: a single run packs
    its arrays back to back, and the driver refuses counts that would misalign its level arrays (the test of the refusal)."""
    return (4,) if shape.startswith("3d") and order == "before" else (3,)


LRS = [0.004, 0.01, 0.02, 0.006, 0.015]


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    saved = odil.util.g_log_file
    odil.util.set_log_file(open(os.devnull, "w"))
    monkeypatch.setenv("ODIL_GRAPH", "0")  # (six epochs never replay; the test of the replay sets it itself)
    yield
    odil.util.g_log_file = saved


def single_runs(build, nb, args, lrs=None):
    """Every member's own `optimize_grad` run: [(reports, x, m, v)] (L-BFGS-B: m, v None; also the optinfo)."""
    results = []
    for b in range(nb):
        problem, state = build(b)
        own = argparse.Namespace(**vars(args))
        own.lr = lrs[b] if lrs is not None else getattr(args, "lr", None)
        seen = []
        callback = lambda state, epoch, pinfo, seen=seen: seen.append((epoch,) + numbers(pinfo))
        try:
            arrays, info = odil.util.optimize_grad(own, args.optimizer, problem, state, callback)
        except EarlyStopError as stop:
            arrays, info = problem.domain.arrays_from_state(state), stop.optinfo
        clone = lambda name: [a.clone() for a in getattr(info, name)] if hasattr(info, name) else None
        results.append((seen, [a.clone() for a in arrays], clone("m"), clone("v"), info))
    return results


def ensemble_run(build, nb, args, form, lrs=None):
    built = [build(b) for b in range(nb)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    seen = [[] for _ in range(nb)]

    def callback(member, state, epoch, pinfo):
        assert state is states[member]
        seen[member].append((epoch,) + numbers(pinfo))

    arrays, info = odil.util.optimize_ensemble(args, problems, states, callback, lrs=lrs, form=form)
    return arrays, info, seen, problems, states


def constants_moved(problems, states, arrays):
    """Every member's `coeff` left its start (half the true constants) in every element the operator reads: equality with
    the single runs is no equality of two runs whose parameter gradient is zero."""
    for b, (problem, state) in enumerate(zip(problems, states)):
        coeff = state.fields["coeff"].array
        assert any(a.data_ptr() == coeff.data_ptr() for a in arrays[b]), "the state's Array is not a view of the returned arrays"
        start = torch.tensor(0.5 * TRUE, dtype=coeff.dtype, device=coeff.device)
        assert bool((coeff.reshape(-1)[:3] != start).all()), (b, list(state.fields), coeff)
        if "mix" in state.fields:
            from param_ensemble_members import MIX

            mix, start = state.fields["mix"].array, torch.tensor(MIX, dtype=coeff.dtype, device=coeff.device)
            assert mix[0, 1] != start[0, 1] and mix[1, 0] != start[1, 0]
            assert mix[0, 0] == start[0, 0] and mix[1, 1] == start[1, 1]  # (never read: no gradient, no step)


# --------------------------------------------------------------------------------------- the ensemble against single runs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,nb,own_lrs,order,mix", RUNS,
                         ids=["{}-B{}-{}-{}{}".format(s, n, "lrs" if o else "lr", r, "-mix" if x else "") for s, n, o, r, x in RUNS])
def test_adam_members_equal_their_single_runs(shape, nb, own_lrs, order, mix, dtype):
    """Six Adam epochs: x of every level AND of every Array, m, v, and every epoch's loss, terms and norms equal the
    members' own `optimize_grad` runs."""
    cshape, nlvl, form = SHAPES[shape]
    args = run_args(epochs=6)
    lrs = LRS[:nb] if own_lrs else None
    build = lambda b: make_member(cshape, nlvl, dtype, b, order=order, mix=mix, coeff_shape=coeff_shape(shape, order))
    singles = [r[:4] for r in single_runs(build, nb, args, lrs)]
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, form if nb != 3 else "auto", lrs)
    assert info.form == form and len(arrays[0]) == (nlvl or 1) + 1 + bool(mix)
    assert_equal_single(arrays, info, seen, problems, states, singles)
    constants_moved(problems, states, arrays)
    assert all(len(report[2]) == 2 and report[4] == ["eq", "data"] for report in seen[0])
    ens = info.ensemble
    assert len(ens.batches) == 1 and ens.batches[0].uploads == 1 and ens.nparams == coeff_shape(shape, order)[0] + 4 * bool(mix)
    assert ens.total == sum(ens.sizes) + ens.nparams
    if nb > 1:
        assert not torch.equal(states[0].fields["coeff"].array, states[1].fields["coeff"].array)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_generated_sources_run_as_two_groups(dtype):
    """Members whose operators differ in a Python constant generate two sources: two groups, each with its own launches
    and its own rows of the packed parameter gradients -- and ONE parameter launch for all of them."""
    nb, (cshape, nlvl, form) = 4, SHAPES["2d-16x24-3lvl"]
    reaction = [1.0, 2.0, 1.0, 2.0]
    args = run_args(epochs=6)
    build = lambda b: make_member(cshape, nlvl, dtype, b, reaction=reaction[b])
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, form, lrs=LRS[:nb])
    assert info.ensemble.groups == [[0, 2], [1, 3]] and len(info.ensemble.batches) == 2
    singles = [r[:4] for r in single_runs(build, nb, args, LRS[:nb])]
    assert_equal_single(arrays, info, seen, problems, states, singles)
    constants_moved(problems, states, arrays)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["2d-16x24-3lvl", "3d-8x8x16-2lvl"])
def test_replayed_epochs_equal_eager_epochs(shape, dtype, monkeypatch):
    cshape, nlvl, form = SHAPES[shape]
    nb, args = 3, run_args(epochs=9)
    build = lambda b: make_member(cshape, nlvl, dtype, b, order="before", coeff_shape=coeff_shape(shape, "before"))
    runs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("ODIL_GRAPH", mode)
        runs.append(ensemble_run(build, nb, args, form, lrs=LRS[:nb]))
    (xa, ia, sa, _, _), (xb, ib, sb, pb, stb) = runs
    assert ia.ensemble.graphable and ib.ensemble.batches[0].uploads == 1
    assert torch.equal(ia.losses, ib.losses) and torch.equal(ia.norms, ib.norms) and sa == sb
    for b in range(nb):
        for got, want in ((xa[b], xb[b]), (ia.m[b], ib.m[b]), (ia.v[b], ib.v[b])):
            assert len(got) == nlvl + 1 and all(torch.equal(p, q) for p, q in zip(got, want))
    constants_moved(pb, stb, xb)


# --------------------------------------------------------------------------------------------------------- L-BFGS-B
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,order", [("2d-16x24-3lvl", "before"), ("3d-8x8x16-2lvl", "after")])
def test_lbfgsb_members_equal_their_single_runs(shape, order, dtype):
    """Twelve iterations in lock-step, bfgs_m = 5: every member ends where its own `lbfgsb` run ends.  The parameter blocks
    stand in the member-major vectors where the single run's packed vector has them (before or after the levels)."""
    cshape, nlvl, form = SHAPES[shape]
    nb, args = 3, run_args("lbfgsb", epochs=12, bfgs_m=5)
    build = lambda b: make_member(cshape, nlvl, dtype, b, order=order)
    singles = single_runs(build, nb, args)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, form)
    assert info.route == "traced" and info.form == form
    assert all(int(n) >= 5 for n in info.nits), info.nits
    for b, (ref_seen, x, _, _, single) in enumerate(singles):
        assert int(info.nits[b]) == int(single.epochs) and int(info.evals[b]) == int(single.evals)
        assert seen[b] == ref_seen, ("reports of member", b)
        final = problems[b].domain.arrays_from_state(states[b])
        for got in (arrays[b], final):
            assert len(got) == len(x)
            for k, (p, q) in enumerate(zip(got, x)):
                assert p.shape == q.shape and torch.equal(p, q), (b, k, float((p - q).abs().max()))
    constants_moved(problems, states, arrays)


def test_elements_that_misalign_a_volume_are_refused():
    """Three Array elements before a 3-D multigrid field: the member's single run would hold its level arrays off the
    alignment its transfer kernels choose by, so the driver refuses it by name and leaves the states alone; four pass (the
    run above), and so do three before a plain 3-D Field (no transfers)."""
    cshape, nlvl, form = SHAPES["3d-8x8x16-2lvl"]
    built = [make_member(cshape, nlvl, np.float64, b, order="before") for b in range(2)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    before = [[(a, a.clone()) for a in p.domain.arrays_from_state(s)] for p, s in built]
    with pytest.raises(ValueError, match="optimize_ensemble: member 0: 3 Array elements stand before the 3-D multigrid field"):
        odil.util.optimize_ensemble(run_args(), problems, states, form=form)
    for (p, s), old in zip(built, before):
        now = p.domain.arrays_from_state(s)
        assert all(a is b and torch.equal(a, copy) for a, (b, copy) in zip(now, old))
    build = lambda b: make_member(cshape, None, np.float64, b, order="before")
    singles = [r[:4] for r in single_runs(build, 2, run_args())]
    assert_equal_single(*ensemble_run(build, 2, run_args(), form), singles)


# ------------------------------------------------------------------------------------------------------ value level
@pytest.mark.parametrize("dtype,tol", [pytest.param(np.float64, 1e-10, id="f64"), pytest.param(np.float32, 2e-5, id="f32")])
@pytest.mark.parametrize("shape", ["2d-16x24-3lvl", "3d-8x8x16-2lvl"])
def test_one_evaluation_against_float64_autograd(shape, dtype, tol, monkeypatch):
    """After ONE evaluation of all members (`loss_grad`): each member's loss and packed parameter gradient against float64
    torch autograd of the same operator on the generic path (tracing off), on the member's own numbers.  The bound is that
    of the single-run checks of generated kernels with `Array` parameters (tests/test_workloads_gpu.py, the `coeff` cases:
    1e-10 in float64, 2e-5 in float32, gradients in the max norm relative to the largest reference gradient entry)."""
    cshape, nlvl, form = SHAPES[shape]
    nb = 3
    built = [make_member(cshape, nlvl, dtype, b, order="around", mix=True) for b in range(nb)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    args = run_args(epochs=0)
    _, info = odil.util.optimize_ensemble(args, problems, states, form=form)
    ens = info.ensemble
    ens.loss_grad()
    torch.cuda.synchronize()
    monkeypatch.setattr(runtime, "enable_trace", False)
    for b in range(nb):
        problem, state = make_member(cshape, nlvl, np.float64, b, order="around", mix=True)
        # (the float64 problem on the member's numbers: float32 inputs widen exactly)
        for name in ("q", "u_obs", "wmask"):
            setattr(problem.extra, name, getattr(problems[b].extra, name).to(torch.float64))
        problem.extra.pfaces = [tuple(p.to(torch.float64) for p in pair) for pair in problems[b].extra.pfaces]
        problem.domain.arrays_to_state([a.to(torch.float64) for a in problems[b].domain.arrays_from_state(states[b])], state)
        loss, grads, _, names, _ = problem.eval_loss_grad(state)
        assert problem._traced is None and names == ["eq", "data"]
        got = ens.levels(ens.g, b)
        scale = max(float(g.abs().max()) for g in grads)
        print("member", b, "loss", float(ens.loss[b]), float(loss), "scale", scale)
        assert abs(float(ens.loss[b]) - float(loss)) <= tol * abs(float(loss))
        kinds = [type(f).__name__ for f in state.fields.values()]
        assert kinds == ["Array", "MultigridField", "Array"]
        for k, (p, q) in enumerate(zip(got, grads)):
            err = float((p.to(torch.float64) - q).abs().max())
            print("  array", k, tuple(q.shape), "error / scale", err / scale)
            assert p.shape == q.shape and err <= tol * scale, (b, k, err / scale)
        assert float(got[-1].abs().min()) > 0 and float(got[0][0, 0]) == 0.0 == float(got[0][1, 1])


# ----------------------------------------------------------------------------------------- ops.adam_step_params_batch
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("npar", [1, 3, 70])
@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("shared", [False, True], ids=["alphas-B", "alpha-1"])
def test_adam_step_params_batch_equals_adam_step_per_member(npar, nb, shared, dtype):
    gen = torch.Generator().manual_seed(17 + npar)
    npg, canary = npar + 2, 1234.5
    draw = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)

    def guarded(values):
        """(the tensor, its buffer with 8 canaries on either side)"""
        buf = torch.full((values.numel() + 16,), canary, dtype=dtype)
        buf[8:-8] = values.reshape(-1)
        buf = buf.cuda()
        return buf[8:-8].view(values.shape), buf

    rows = torch.randperm(npg, generator=gen)[:npar].tolist()
    if npar > 1:
        rows[1] = -1  # (no grid gradient: g = 0)
    if npar == 70:
        rows[40:44] = [-1] * 4
    (x, xbuf), (m, mbuf), (g, gbuf) = guarded(draw(nb, npar)), guarded(draw(nb, npar)), guarded(draw(nb, npar))
    v, vbuf = guarded(draw(nb, npar).abs())
    pgrad = draw(nb, npg).cuda()
    index = ops.param_rows(rows, npg, "cuda")
    alphas = torch.tensor([0.01] if shared else [0.01, 0.02, 0.005, 0.03, 0.001][:nb], dtype=dtype).cuda()
    omb1, omb2, eps = 1 - np.float64(0.9), 1 - np.float64(0.999), 1e-7
    permuted = torch.stack([torch.stack([pgrad[b, r] if r >= 0 else torch.zeros((), dtype=dtype, device="cuda") for r in rows])
                            for b in range(nb)])
    want = []
    for b in range(nb):
        xs, ms, vs = (t[b].clone() for t in (x, m, v))
        ops.adam_step(xs, ms, vs, permuted[b].clone(), alphas[0 if shared else b:][:1], omb1, omb2, eps)
        want.append((xs, ms, vs))
    # the gradient-only mode: x, m, v untouched
    before = [t.clone() for t in (xbuf, mbuf, vbuf)]
    ops.adam_step_params_batch(None, None, None, g, pgrad, index)
    assert torch.equal(g, permuted) and all(torch.equal(now, old) for now, old in zip((xbuf, mbuf, vbuf), before))
    g.fill_(7.0)
    ops.adam_step_params_batch(x, m, v, g, pgrad, index, alphas, omb1, omb2, eps)
    assert torch.equal(g, permuted)
    for b in range(nb):
        for got, ref in zip((x, m, v), want[b]):
            assert torch.equal(got[b], ref)
    assert not torch.equal(x[0], before[0][8:8 + npar])
    for buf in (xbuf, mbuf, vbuf, gbuf):  # the canaries behind (and before) the buffers
        assert bool((buf[:8] == canary).all()) and bool((buf[-8:] == canary).all())
    # a map per member gives the same
    g.fill_(7.0)
    ops.adam_step_params_batch(None, None, None, g, pgrad, ops.param_rows([rows] * nb, npg, "cuda"))
    assert torch.equal(g, permuted)
    with pytest.raises(ValueError, match="param_rows"):
        ops.param_rows([npg], npg, "cuda")


# ------------------------------------------------------------------------------------------- forward members unchanged
def test_forward_members_issue_the_launches_they_issued(monkeypatch):
    """Members WITHOUT Array unknowns: per epoch the library calls of `TracedLaunchEnsemble.epoch` as before, and not one
    call of the new entry point."""
    from odil_amd import _lib

    cshape, nlvl, form = SHAPES["2d-16x24-3lvl"]
    built = [make_member(cshape, nlvl, np.float64, b, operator_=forward_only) for b in range(3)]
    called, real = [], _lib.call

    def counting(name, *args, **kwargs):
        called.append(name)
        return real(name, *args, **kwargs)

    params = []
    monkeypatch.setattr(ops, "call", counting)
    monkeypatch.setattr(ops, "adam_step_params_batch", lambda *a, **k: params.append(a))
    _, info = odil.util.optimize_ensemble(run_args(epochs=3), [p for p, _ in built], [s for _, s in built], form=form)
    assert info.route == "traced" and info.ensemble.nparams == 0 and type(info.ensemble.x) is list
    assert params == [] and "adam_step_params_batch" not in called
    epoch = ["mg_synth", "mg_synth_adj_adam_members", "adam_step_batch"]
    assert [name for name in called if name in epoch or "adam" in name][-9:] == epoch * 3
