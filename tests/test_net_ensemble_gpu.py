"""Ensembles of inverse problems with `NeuralNet` unknowns and outputs in parameter space on the device:
`odil.util.optimize_ensemble` for members like examples/heat (`fused.TracedLaunchEnsemble` with the networks' arrays in the
packed parameters, `stencil_bind.EpochBatch`, the generated `k_par_batch`, `ops.adam_step_params_batch(extra=...)`).  Every
member -- field, network weights and biases, Arrays, moments, every epoch's loss, terms, norms and names -- must end where
its own `optimize_grad` run ends, bit for bit (`torch.equal`), with Adam and with L-BFGS-B, in float64 and in float32; member
0 built from the reference's fixtures follows the reference's own Adam trajectory to the tolerances the single run is held
to.  Members: tests/net_ensemble_members.py."""

import argparse
import os

import numpy as np
import pytest
import torch
from net_ensemble_members import FORMS, advance_epoch, make_member, run_args
from test_traced_ensemble_gpu import assert_equal_single, ensemble_run, numbers, single_runs

import odil_amd as odil
from odil_amd import ops
from odil_amd.optimizer import EarlyStopError

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
LRS = [0.004, 0.01, 0.02, 0.006, 0.015]
NPAR = 46
# (members, operator, dtype, B, form, a step size per member, order of the state): each shape in both dtypes, with heat's own
# operator (wreg: identically zero) and with the live priors, B = 1, 3 and 5, one 2-D case with the network before the field
ADAM_RUNS = [
    ("heat", "heat", F64, 3, "auto", False, "after"),
    ("heat", "live", F32, 5, "launches", True, "after"),
    ("heat", "live", F64, 1, "launches", False, "after"),
    ("heat2d", "live", F64, 3, "volumes", False, "after"),
    ("heat2d", "heat", F32, 1, "volumes", False, "after"),
    ("plain", "live", F64, 3, "launches", False, "before"),
    ("plain", "heat", F32, 5, "launches", False, "after"),
]


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    saved = odil.util.g_log_file
    odil.util.set_log_file(open(os.devnull, "w"))
    monkeypatch.setenv("ODIL_GRAPH", "0")  # (the test of the replay sets it itself)
    yield
    odil.util.g_log_file = saved


def network_arrays(problem, state):
    return problem.domain.arrays_from_field(state.fields["k_net"])


def moved_and_distinct(build, problems, states, arrays):
    """Every member's weights and biases left their start, are views of the returned arrays, and members differ."""
    for b, (problem, state) in enumerate(zip(problems, states)):
        start = network_arrays(*build(b))
        now = network_arrays(problem, state)
        assert len(now) == 6 and all(any(a.data_ptr() == w.data_ptr() for a in arrays[b]) for w in now)
        assert all(not torch.equal(w, w0) for w, w0 in zip(now, start)), ("weights of member", b, "did not move")
        if "c" in state.fields:
            c0, c = build(b)[1].fields["c"].array, state.fields["c"].array
            assert bool((c != c0).all()), ("constants of member", b, c, c0)
    if len(states) > 1:
        assert not torch.equal(network_arrays(problems[0], states[0])[1], network_arrays(problems[1], states[1])[1])


def terms_named(seen, name):
    """The term `name` of every report of one member after the start."""
    return [report[2][report[4].index(name)] for report in seen[1:]]


# --------------------------------------------------------------------------------------------------- 5: Adam, bit identity
@pytest.mark.parametrize("which,operator,dtype,nb,form,own_lrs,order", ADAM_RUNS, ids=[
    "{}-{}-{}-B{}-{}-{}".format(w, o, "f64" if d is F64 else "f32", n, f, r) for w, o, d, n, f, _, r in ADAM_RUNS])
def test_adam_members_equal_their_single_runs(which, operator, dtype, nb, form, own_lrs, order):
    """Six Adam epochs, both sides advancing the `epoch` tracer in their callbacks: everything equals the members' own runs."""
    args = run_args(epochs=6)
    lrs = LRS[:nb] if own_lrs else None
    build = lambda b: make_member(which, dtype, b, operator=operator, order=order)
    singles = single_runs(build, nb, args, lrs, tracer_plan=advance_epoch)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, form, lrs, tracer_plan=advance_epoch)
    assert info.form == FORMS[which]
    nlvl = 1 if which == "plain" else 3
    assert len(arrays[0]) == nlvl + 6 + (operator == "live")
    assert_equal_single(arrays, info, seen, problems, states, singles)
    moved_and_distinct(build, problems, states, arrays)
    ens = info.ensemble
    assert len(ens.batches) == 1 and ens.nparams == NPAR + 4 * (operator == "live") and ens.total == sum(ens.sizes) + ens.nparams
    assert not ens.graphable and ens.batches[0].uploads == 6  # (annealed terms: the blocks are staged again every epoch)
    for b in range(nb):
        names = seen[b][0][4]
        if operator == "live":
            assert names[-2:] == ["wdecay", "cprior"]
            assert all(t > 0 for t in terms_named(seen[b], "wdecay")) and all(t > 0 for t in terms_named(seen[b], "cprior"))
            decay = terms_named(seen[b], "wdecay")
            assert decay[-1] < decay[0]  # (annealed: 0.5 ** (epoch / 4))
        elif which != "heat2d":
            assert names[-1] == "wreg" and all(t == 0 for t in terms_named(seen[b], "wreg"))
    if operator == "live":
        assert ens.gextra is not None and float(ens.gextra.params.abs().max()) == 0.0  # (cleared by the parameter launch)
        rows = ens.param_rows.cpu().tolist()
        assert sorted(r for r in rows if r >= 0) == list(range(NPAR + 4))


# ------------------------------------------------------------------------------------------------- 6: reference anchor
LOSS_RTOL = dict(f64=1e-12, f32=2e-5)  # what tests/test_traj_workloads_gpu.py holds the single run's losses to


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("which", ["heat", "heat2d"])
def test_member_from_the_fixture_follows_the_reference(which, tag):
    """B = 3, member 0 built from the fixture as the single-run test builds it, the others with perturbed networks: ten free
    epochs from the reference's state at epoch 1 against its state at epoch 11 and its loss of every epoch."""
    from conftest import load_golden
    from test_traj_workloads_gpu import build, check_state, state_at

    t = load_golden("traj_adam_states_{}_{}".format(which, tag))
    lr = float(t["lr"])
    mod = odil.runtime.get_mod()
    problems, states = [], []
    for b in range(3):
        problem, state, n = build(which, tag)
        x = [mod.array(a) for a in state_at(t, 1, n)[0]]
        if b:
            gen = torch.Generator().manual_seed(b)
            x = x[:-6] + [a + 0.05 * torch.randn(a.shape, generator=gen, dtype=torch.float64).to(a.dtype).to(a.device) for a in x[-6:]]
        problem.domain.arrays_to_state(x, state)
        problem.tracers["epoch"] = 1
        problems.append(problem)
        states.append(state)

    def callback(member, state, epoch, pinfo):
        problems[member].tracers["epoch"] = epoch + 1

    args = run_args(epochs=10, lr=lr)
    arrays, info = odil.util.optimize_ensemble(args, problems, states, callback, form=FORMS[which])
    assert info.route == "traced" and len(arrays[0]) == n
    check_state((arrays[0], info.m[0], info.v[0]), state_at(t, 11, n), tag, lr, "free")
    losses = info.losses[0].cpu().numpy()
    for k in range(10):
        ref = float(t["losses"][k])
        print("epoch", k + 1, "loss", float(losses[k]), "reference", ref)
        assert abs(float(losses[k]) - ref) <= LOSS_RTOL[tag] * abs(ref), (k, float(losses[k]), ref)
    assert not torch.equal(arrays[0][-6], arrays[1][-6])


# --------------------------------------------------------------------------------------------------------- 7: L-BFGS-B
def lbfgsb_single_runs(build, nb, args):
    results = []
    for b in range(nb):
        problem, state = build(b)
        seen = []
        callback = lambda state, epoch, pinfo, seen=seen: seen.append((epoch,) + numbers(pinfo))
        try:
            arrays, info = odil.util.optimize_grad(argparse.Namespace(**vars(args)), "lbfgsb", problem, state, callback)
        except EarlyStopError as stop:
            arrays, info = problem.domain.arrays_from_state(state), stop.optinfo
        results.append((seen, [a.clone() for a in arrays], info))
    return results


@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
def test_lbfgsb_members_equal_their_single_runs(dtype):
    """Twelve iterations in lock-step, bfgs_m = 5, the live priors: every member ends where its own `lbfgsb` run ends."""
    nb, args = 3, run_args("lbfgsb", epochs=12, bfgs_m=5)
    build = lambda b: make_member("heat", dtype, b, operator="live")
    singles = lbfgsb_single_runs(build, nb, args)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "launches")
    assert info.route == "traced" and info.form == "launches"
    for b, (ref_seen, x, single) in enumerate(singles):
        assert int(info.nits[b]) == int(single.epochs) and int(info.evals[b]) == int(single.evals)
        assert info.tasks[b] == single.task, (b, info.tasks[b], single.task)
        assert seen[b] == ref_seen, ("reports of member", b)
        final = problems[b].domain.arrays_from_state(states[b])
        for got in (arrays[b], final):
            assert len(got) == len(x) == 3 + 6 + 1
            for k, (p, q) in enumerate(zip(got, x)):
                assert p.shape == q.shape and torch.equal(p, q), (b, k, float((p - q).abs().max()))
    assert all(int(n) >= 3 for n in info.nits), info.nits
    moved_and_distinct(build, problems, states, arrays)


# ----------------------------------------------------------------------------------------------------------- 8: groups
def test_two_activations_run_as_two_groups(monkeypatch):
    """Four members, two network architectures of the same layer shapes (tanh and relu: the layer shapes must agree, they
    are the packed layout): two generated sources, two groups, each with its own rows of the packed parameter gradients and
    its own `k_par_batch` -- and ONE parameter launch per epoch for all of them."""
    nb, activation = 4, ["tanh", "relu", "tanh", "relu"]
    args = run_args(epochs=6)
    build = lambda b: make_member("heat", F64, b, operator="live", activation=activation[b])
    singles = single_runs(build, nb, args, LRS[:nb], tracer_plan=advance_epoch)
    calls, real = [], ops.adam_step_params_batch
    monkeypatch.setattr(ops, "adam_step_params_batch", lambda *a, **k: (calls.append(k.get("extra") is not None), real(*a, **k))[1])
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "launches", LRS[:nb], tracer_plan=advance_epoch)
    ens = info.ensemble
    assert ens.groups == [[0, 2], [1, 3]] and len(ens.batches) == 2 and len(ens.par_batches) == 2
    assert calls == [True] * 6
    assert_equal_single(arrays, info, seen, problems, states, singles)
    moved_and_distinct(build, problems, states, arrays)


# --------------------------------------------------------------------------------------------------- 9: frozen network
def test_frozen_network_gets_its_gradient_set_not_added():
    """The network is read only with frozen=True and regularised: no grid kernel writes its gradient (`param_rows` -1), the
    parameter kernel SETS it.  Adding would show from the second epoch on."""
    nb, args = 3, run_args(epochs=6)
    build = lambda b: make_member("heat", F64, b, operator="frozen")
    singles = single_runs(build, nb, args, tracer_plan=advance_epoch)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "launches", tracer_plan=advance_epoch)
    ens = info.ensemble
    assert ens.param_rows.cpu().tolist() == [-1] * NPAR and "k_net" not in ens.traced[0].cg.pgrads
    assert_equal_single(arrays, info, seen, problems, states, singles)
    moved_and_distinct(build, problems, states, arrays)
    assert all(t > 0 for t in terms_named(seen[0], "wdecay"))


# --------------------------------------------------------------------------------------------------- 10: launch staging
def test_members_without_host_scalars_are_staged_once_and_replayed(monkeypatch):
    """A network and a weight decay but no tracer: the blocks (the `ParArgs` among them) are staged once, the epochs may be
    replayed as a graph, and the replayed run equals the (eager) single runs."""
    nb, args = 3, run_args(epochs=9)
    build = lambda b: make_member("heat", F64, b, operator="constant", annealed=False)
    singles = single_runs(build, nb, args, LRS[:nb])
    monkeypatch.setenv("ODIL_GRAPH", "1")
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "launches", LRS[:nb])
    ens = info.ensemble
    assert ens.graphable and ens.batches[0].uploads == 1 and ens.batches[0].npar_out == 2
    assert_equal_single(arrays, info, seen, problems, states, singles)
    assert all(t > 0 for t in terms_named(seen[0], "wdecay"))


def test_blocks_are_staged_again_only_when_a_host_scalar_changed():
    """The annealed term: the tracer advances after epochs 1, 2 and 4 only -- four uploads in six epochs."""
    nb, args = 2, run_args(epochs=6)
    plan = lambda problem, epoch: problem.tracers.__setitem__("epoch", {0: 1, 1: 2, 2: 3, 3: 3, 4: 5, 5: 5, 6: 5}[epoch])
    build = lambda b: make_member("heat", F64, b, operator="live")
    singles = single_runs(build, nb, args, tracer_plan=plan)
    arrays, info, seen, problems, states = ensemble_run(build, nb, args, "launches", tracer_plan=plan)
    assert info.ensemble.batches[0].uploads == 4 and info.ensemble.batches[0].launches == 6
    assert_equal_single(arrays, info, seen, problems, states, singles)


# ------------------------------------------------------------------------------------------------------- 11: refusals
def untouched(build, nb, match, form, **kwargs):
    built = [build(b) for b in range(nb)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    before = [[(a, a.clone()) for a in p.domain.arrays_from_state(s)] for p, s in built]
    with pytest.raises(ValueError, match=match):
        odil.util.optimize_ensemble(run_args(), problems, states, form=form, **kwargs)
    for (p, s), old in zip(built, before):
        now = p.domain.arrays_from_state(s)
        assert len(now) == len(old) and all(a is b and torch.equal(a, copy) for a, (b, copy) in zip(now, old))


def test_refusals_on_the_device_leave_the_states_alone(monkeypatch):
    # a network before a 3-D multigrid field: 46 elements are no multiple of 4
    untouched(lambda b: make_member("heat2d", F64, b, order="before"), 2,
              "optimize_ensemble: member 0: 46 Array and NeuralNet elements stand before the 3-D multigrid field", "volumes")
    # a parameter output that only the torch replay evaluates
    untouched(lambda b: make_member("heat", F64, b, operator="torch"), 2, "member 0: .*evaluated by torch", "launches")
    # a member forced to march
    monkeypatch.setenv("ODIL_TRACE_SHARE", "march")
    untouched(lambda b: make_member("heat2d", F32, b), 2, "member 0: .*marching", "volumes")
