"""Adam ensembles of traced stencil operators on the device (`odil.util.optimize_ensemble` with form 'launches' / 'volumes' /
'auto' for members that are not the Poisson stencil: `fused.TracedLaunchEnsemble`, `stencil_bind.EpochBatch`, the generated
`k_fwd_batch` / `k_gat_*_batch`, `ops.adam_step_batch`).  Every member must end where its own `optimize_grad(args, "adam", ...)`
run ends, bit for bit (`torch.equal`), in float64 and in float32.  Members differ in conductivity amplitude, right-hand side
and initial guess, all seeded (tests/traced_ensemble_members.py)."""

import argparse
import os

import numpy as np
import pytest
import torch
from traced_ensemble_members import diffusion_ensemble, make_member, make_members, run_args, two_outputs

import odil_amd as odil
from odil_amd import ops, runtime

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")]
# (cells, levels of the MultigridField or None for a plain Field, form)
SHAPES = dict([
    ("1d-64-3lvl", ((64,), 3, "launches")),
    ("2d-16-3lvl", ((16, 16), 3, "launches")),
    ("2d-12x18-odd-rows", ((12, 18), 2, "launches")),  # (rows no multiple of 4: one point per thread; coarse rows odd)
    ("3d-8-2lvl", ((8, 8, 8), 2, "volumes")),
    ("2d-16-plain-field", ((16, 16), None, "launches")),
    ("2d-8x512-interior", ((8, 512), 2, "launches")),
])
# every shape with beta = 0 or beta = 1 and with a shared or a per-member step size; both operators and both kinds of step
# size on the 2-D and the 3-D multigrid members (every distinct operator, shape and dtype is one more generated library)
RUNS = [("1d-64-3lvl", 0.0, False), ("2d-16-3lvl", 0.0, False), ("2d-16-3lvl", 1.0, True), ("2d-12x18-odd-rows", 1.0, True),
        ("3d-8-2lvl", 0.0, True), ("3d-8-2lvl", 1.0, False), ("2d-16-plain-field", 1.0, True), ("2d-16-plain-field", 0.0, False),
        ("2d-8x512-interior", 0.0, False), ("2d-8x512-interior", 1.0, True)]


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    saved = odil.util.g_log_file
    odil.util.set_log_file(open(os.devnull, "w"))
    monkeypatch.setenv("ODIL_GRAPH", "0")  # (three epochs never replay; the tests of the replay set it themselves)
    yield
    odil.util.g_log_file = saved


def numbers(pinfo):
    """(loss, terms, norms, names) of a callback's report as host numbers (exact: float32 widens without rounding)."""
    value = lambda t: float(np.array(t))
    return value(pinfo["loss"]), [value(t) for t in pinfo["terms"]], [value(t) for t in pinfo["norms"]], list(pinfo["names"])


def single_runs(build, nb, args, lrs=None, tracer_plan=None):
    """Every member's own `optimize_grad` run: [(reports per epoch, x, m, v)].  build(b) -> (problem, state)."""
    results = []
    for b in range(nb):
        problem, state = build(b)
        own = argparse.Namespace(**vars(args))
        own.lr = lrs[b] if lrs is not None else args.lr
        seen = []

        def callback(state, epoch, pinfo, seen=seen, problem=problem):
            seen.append((epoch,) + numbers(pinfo))
            if tracer_plan is not None:
                tracer_plan(problem, epoch)

        arrays, info = odil.util.optimize_grad(own, "adam", problem, state, callback)
        results.append((seen, [a.clone() for a in arrays], [a.clone() for a in info.m], [a.clone() for a in info.v]))
    return results


def ensemble_run(build, nb, args, form, lrs=None, tracer_plan=None, members=None):
    members = list(range(nb)) if members is None else members
    built = [build(b) for b in members]
    problems, states = [p for p, _ in built], [s for _, s in built]
    seen = [[] for _ in members]

    def callback(member, state, epoch, pinfo):
        assert state is states[member]
        seen[member].append((epoch,) + numbers(pinfo))
        if tracer_plan is not None:
            tracer_plan(problems[member], epoch)

    arrays, info = odil.util.optimize_ensemble(args, problems, states, callback, lrs=lrs, form=form)
    return arrays, info, seen, problems, states


def assert_equal_single(arrays, info, seen, problems, states, singles, members=None):
    members = list(range(len(singles))) if members is None else members
    assert info.route == "traced" and len(arrays) == len(members)
    assert torch.equal(info.norms, torch.sqrt(info.losses))
    for j, b in enumerate(members):
        ref_seen, x, m, v = singles[b]
        assert seen[j] == ref_seen, ("reports of member", b, seen[j], ref_seen)
        for epoch, loss, _, _, _ in ref_seen[1:]:  # (epoch 0 is the report of the start)
            assert float(info.losses[j, epoch - 1]) == loss
        final = problems[j].domain.arrays_from_state(states[j])
        for name, got, want in (("x", arrays[j], x), ("m", info.m[j], m), ("v", info.v[j], v), ("state", final, x)):
            assert len(got) == len(want)
            for lvl, (p, q) in enumerate(zip(got, want)):
                assert p.shape == q.shape and torch.equal(p, q), (b, name, lvl, float((p - q).abs().max()))


# --------------------------------------------------------------------------------------- the ensemble against single runs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,beta,own_lrs", RUNS, ids=["{}-beta{:.0f}-{}".format(s, b, "lrs" if o else "lr") for s, b, o in RUNS])
def test_members_equal_their_single_runs(shape, beta, own_lrs, dtype):
    """Three members, three epochs: x of every level, m, v, and every epoch's loss, terms and norms equal the members' own
    `optimize_grad` runs.  beta = 1: the gather re-reads its sources; own_lrs: a step size per member.

    The shape 8 x 512 -> 4 x 256 is the one where wavefronts take the INTERIOR copy of the forward body: four points of
    the last axis per thread, so a wavefront holds 256 consecutive cells = half a row, all on one i0, and the interior
    condition of the generated source (`__all(i0 >= 1 && i0 <= 6)`, the last axis is not folded at four points per thread)
    holds for the wavefronts of rows 1 ... 6 and fails for those of rows 0 and 7.  (At 16 x 16 one wavefront holds the
    whole grid and none is interior; at 12 x 18 a wavefront of 64 single points always meets a wall.)"""
    nb = 3
    cshape, nlvl, form = SHAPES[shape]
    args = run_args(epochs=3)
    lrs = [0.004, 0.01, 0.02] if own_lrs else None
    build = lambda b: make_member(cshape, nlvl, dtype, b, nb, beta=beta)
    singles = single_runs(build, nb, args, lrs)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, form, lrs)
    assert info.form == form and len(arrays[0]) == (nlvl or 1)
    assert_equal_single(arrays, info, seen, problems, states, singles)
    assert not torch.equal(arrays[0][0], arrays[1][0])
    ens = info.ensemble
    assert len(ens.batches) == 1 and ens.batches[0].uploads == 1  # (one group, its blocks staged once)
    if cshape == (8, 512):
        assert "if (__all((int)(i0 >= 1 && i0 <= 6))) {" in ens.traced[0].source and ens.traced[0].cg.vw_fwd == 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["2d-16-3lvl", "3d-8-2lvl"])
def test_two_outputs_with_different_weights(shape, dtype):
    """An operator with TWO outputs (`two_outputs`): k_final_batch / k_loss_batch reduce two rows per member, the loss is
    their sum, and the callback reports both terms and norms under the member's own names."""
    nb = 3
    cshape, nlvl, form = SHAPES[shape]
    args = run_args(epochs=3)
    build = lambda b: make_member(cshape, nlvl, dtype, b, nb, beta=0.5, operator=two_outputs)
    singles = single_runs(build, nb, args)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "auto")
    assert info.form == form and info.ensemble.traced[0].nout == 2
    assert all(len(report[2]) == 2 and len(report[3]) == 2 for report in seen[0])
    assert_equal_single(arrays, info, seen, problems, states, singles)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_member_equals_five(dtype):
    """B = 1 and B = 5 give the same bits for member 0 (and both the single run's)."""
    nb, cshape, nlvl = 5, (16, 16), 3
    args = run_args(epochs=3)
    build = lambda b: make_member(cshape, nlvl, dtype, b, nb, beta=1.0)
    singles = single_runs(build, 1, args)
    five = ensemble_run(build, nb, args, "launches")
    one = ensemble_run(build, nb, args, "launches", members=[0])
    assert_equal_single(*one, singles, members=[0])
    for got, want in ((one[0][0], five[0][0]), (one[1].m[0], five[1].m[0]), (one[1].v[0], five[1].v[0])):
        assert all(torch.equal(p, q) for p, q in zip(got, want))
    assert torch.equal(one[1].losses[0], five[1].losses[0]) and one[2][0] == five[2][0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_generated_sources_run_as_two_groups(dtype):
    """Members at beta = 0 and beta = 1 generate two different sources: two groups, one launch of each kernel per group,
    the losses collected from two packed `out` tensors -- and still the single runs' bits."""
    nb, cshape, nlvl = 4, (16, 16), 3
    betas = [0.0, 1.0, 0.0, 1.0]
    args = run_args(epochs=3)
    build = lambda b: make_member(cshape, nlvl, dtype, b, nb, beta=betas[b])
    lrs = [0.01, 0.005, 0.02, 0.01]
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "launches", lrs=lrs)
    assert info.ensemble.groups == [[0, 2], [1, 3]] and len(info.ensemble.batches) == 2
    singles = single_runs(build, nb, args, lrs=lrs)
    assert_equal_single(arrays, info, seen, problems, states, singles)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["2d-16-3lvl", "3d-8-2lvl", "2d-16-plain-field"])
def test_replayed_epochs_equal_eager_epochs(shape, dtype, monkeypatch):
    """ODIL_GRAPH=1 (two eager epochs, then the epoch replayed as a captured graph: a chain on one stream) and ODIL_GRAPH=0
    give the same bits."""
    nb = 3
    cshape, nlvl, form = SHAPES[shape]
    args = run_args(epochs=9)
    build = lambda b: make_member(cshape, nlvl, dtype, b, nb, beta=1.0)
    runs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("ODIL_GRAPH", mode)
        runs.append(ensemble_run(build, nb, args, form, lrs=[0.004, 0.01, 0.02]))
    (xa, ia, sa, _, _), (xb, ib, sb, _, _) = runs
    assert ia.ensemble.graphable and ib.ensemble.batches[0].uploads == 1
    assert torch.equal(ia.losses, ib.losses) and torch.equal(ia.norms, ib.norms) and sa == sb
    for b in range(nb):
        for got, want in ((xa[b], xb[b]), (ia.m[b], ib.m[b]), (ia.v[b], ib.v[b])):
            assert all(torch.equal(p, q) for p, q in zip(got, want))
    assert float(ia.losses[0, -1]) != float(ia.losses[0, 0])


# -------------------------------------------------------------------------------------------------------- host scalars
def weighted(ctx):
    """The example's operator times a weight that is a function of a tracer: a host scalar of the trace."""
    return [diffusion_ensemble().operator(ctx)[0] * (1.0 + ctx.tracers["w"])]


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_scalar_that_changes_between_epochs_is_uploaded_again(dtype, monkeypatch):
    """The tracer of members 1 and 2 changes after the first epoch (in the callback, as a schedule would): the next epoch evaluates
    with the new weight, as the member's single run does -- the argument blocks are staged again for that epoch, and not
    for the one after it, where nothing changes.  Such an ensemble is never replayed as a graph."""
    nb, cshape, nlvl = 3, (16, 16), 3
    args = run_args(epochs=8)

    def build(b):
        problem, state = make_member(cshape, nlvl, dtype, b, nb, beta=1.0, operator=weighted)
        problem.tracers, problem.member = dict(w=0.0), b
        return problem, state

    def plan(problem, epoch):  # (member 0 keeps its weight, the others change it)
        if problem.member != 0 and epoch == 1:
            problem.tracers["w"] = 0.5

    monkeypatch.setenv("ODIL_GRAPH", "0")
    singles = single_runs(build, nb, args, tracer_plan=plan)
    monkeypatch.setenv("ODIL_GRAPH", "1")
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "launches", tracer_plan=plan)
    assert not info.ensemble.graphable and info.ensemble.batches[0].hs_members == [0, 1, 2]
    assert info.ensemble.batches[0].uploads == 2
    assert_equal_single(arrays, info, seen, problems, states, singles)
    # the weight entered: a run that never changes it differs from epoch 2 on
    still = ensemble_run(build, nb, args, "launches")
    assert torch.equal(still[1].losses[:, 0], info.losses[:, 0]) and torch.equal(still[1].losses[0], info.losses[0])
    assert not torch.equal(still[1].losses[1:, 1], info.losses[1:, 1])


# ------------------------------------------------------------------------------------------------------------ refusals
def _arrays(state):
    return [getattr(box, at) if isinstance(at, str) else box[at] for f in state.fields.values()
            for box, at in odil.core.Domain._slots(f)]


def refused(args, problems, states, match, **kwargs):
    """The call raises ValueError(match) and leaves every state's arrays in place with their values."""
    before = [[(a, a.detach().clone()) for a in _arrays(s)] for s in states]
    with pytest.raises(ValueError, match=match):
        odil.util.optimize_ensemble(args, problems, states, **kwargs)
    for s, old in zip(states, before):
        now = _arrays(s)
        assert len(now) == len(old) and all(p is a and torch.equal(p.detach(), copy) for p, (a, copy) in zip(now, old))


def test_refusals_leave_the_states_untouched(monkeypatch):
    args, dtype = run_args(), np.float64
    problems, states = make_members((16, 16), 3, dtype, 3)
    poisson = "member 0: the operator is not the recognised Poisson stencil"
    refused(args, problems, states, poisson, form="workgroup")
    refused(args, problems, states, poisson)  # (the default form)
    monkeypatch.setattr(runtime, "enable_trace", False)
    fresh = make_members((16, 16), 3, dtype, 3)  # (nothing probed yet: recognised with tracing off)
    refused(args, *fresh, poisson, form="launches")
    monkeypatch.setattr(runtime, "enable_trace", True)
    # a member with a network unknown
    net = make_member((16, 16), 3, dtype, 1, 3)
    net[1].fields.clear()
    net[1].fields["u"] = net[0].domain.init_field(net[0].domain.make_neural_net([2, 4, 1]))
    refused(args, [problems[0], net[0]], [states[0], net[1]], "member 1: the unknown is not a cell-centred field", form="launches")
    # two unknowns
    two = make_member((16, 16), 3, dtype, 1, 3)
    two[1].fields["w"] = two[0].domain.init_field(None)
    refused(args, [problems[0], two[0]], [states[0], two[1]], "member 1: 2 unknown fields", form="launches")
    # non-unit multigrid factors
    scaled = make_member((16, 16), 3, dtype, 1, 3, mg_factors=[1.0, 2.0, 4.0])
    refused(args, [problems[0], scaled[0]], [states[0], scaled[1]], r"member 1: multigrid factors \[1.0, 2.0, 4.0\]", form="launches")
    # a differing cshape
    other = make_member((16, 32), 3, dtype, 2, 3)
    refused(args, problems[:2] + [other[0]], states[:2] + [other[1]], "member 2: level shapes .* differ from member 0's", form="auto")
    # the members the refusals named run once they stand among their like
    arrays, info = odil.util.optimize_ensemble(args, problems, states, form="auto")
    assert info.route == "traced" and info.form == "launches"


# ------------------------------------------------------------------------------------------------ ops.adam_step_batch
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,pad", [((12, 18), 0), ((12, 18), 3), ((7,), 1), ((8, 8, 8), 0), ((4100,), 4)],
                         ids=["2d", "2d-padded", "1d-odd-padded", "3d", "1d-two-blocks-padded"])
@pytest.mark.parametrize("shared", [False, True], ids=["alphas-B", "alpha-1"])
def test_adam_step_batch_equals_adam_step_per_member(shape, pad, shared, dtype):
    nb, cells = 5, int(np.prod(shape))
    gen = torch.Generator().manual_seed(5)

    def members(positive=False):
        base = torch.randn(nb * (cells + pad), generator=gen, dtype=torch.float64)
        base = (base.abs() if positive else base).to(dtype).cuda()
        strides = [int(np.prod(shape[k + 1:])) for k in range(len(shape))]
        return base, base.as_strided((nb,) + tuple(shape), [cells + pad] + strides)

    (xb, x), (mb, m), (vb, v), (gb, g) = members(), members(), members(True), members()
    alphas = torch.tensor([0.01] if shared else [0.01, 0.02, 0.005, 0.03, 0.001], dtype=dtype).cuda()
    omb1, omb2, eps = 1 - np.float64(0.9), 1 - np.float64(0.999), 1e-7
    want = []
    for b in range(nb):
        xs, ms, vs = (t[b].clone().view(-1) for t in (x, m, v))
        ops.adam_step(xs, ms, vs, g[b].clone().view(-1), alphas[0 if shared else b:][:1], omb1, omb2, eps)
        want.append((xs, ms, vs))
    bases = [t.clone() for t in (xb, mb, vb)]
    ops.adam_step_batch(x, m, v, g, alphas, omb1, omb2, eps)
    for b in range(nb):
        for got, ref in zip((x, m, v), want[b]):
            assert torch.equal(got[b].reshape(-1), ref)
    if pad:  # the elements between the members are not touched
        gap = torch.ones(cells + pad, dtype=torch.bool)
        gap[:cells] = False
        gap = gap.repeat(nb).cuda()
        for now, old in zip((xb, mb, vb), bases):
            assert torch.equal(now[gap], old[gap])
    assert not torch.equal(x[0].reshape(-1), bases[0][:cells])


# ------------------------------------------------------------------------------------- the Poisson ensembles stay as they were
def test_poisson_members_keep_their_route_and_their_launches(monkeypatch):
    """Members that are all the recognised Poisson stencil do not take the traced route: `form="launches"` makes, per
    epoch, exactly the four library calls of `fused.PoissonLaunchEnsemble.epoch` and no generated kernel is loaded."""
    import sys

    from conftest import ROOT

    from odil_amd import _lib, fused, stencil_jit

    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    pargs = poisson.parse_args("--ndim 2 --N 16".split())
    pargs.epoch_start, pargs.epochs = 0, 3
    built = [poisson.make_problem(pargs) for _ in range(2)]
    called, real = [], _lib.call

    def counting(name, *args, **kwargs):
        called.append(name)
        return real(name, *args, **kwargs)

    def no_trace(*args, **kwargs):
        raise AssertionError("a Poisson member was traced")

    arrays = built[0][0].domain.arrays_from_state(built[0][1])
    assert fused.launches_refusal([tuple(a.shape) for a in arrays], arrays[0].dtype) is None
    monkeypatch.setattr(ops, "call", counting)
    monkeypatch.setattr(stencil_jit, "TracedOperator", no_trace)
    _, info = odil.util.optimize_ensemble(pargs, [p for p, _ in built], [s for _, s in built], form="launches")
    assert info.route == "poisson" and info.form == "launches" and type(info.ensemble) is fused.PoissonLaunchEnsemble
    epoch = ["mg_synth", "poisson_residual_batch", "poisson_adjoint_adam_batch", "mg_synth_adj_adam_members"]
    assert called[-12:] == epoch * 3  # (ahead of them: the probes of `fused.detect`, nothing of an epoch)
    assert not [name for name in called[:-12] if name in epoch or "adam" in name]
