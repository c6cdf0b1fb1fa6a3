#!/usr/bin/env python3
"""A sweep of the inverse heat-conduction problem of heat.py (`--infer_k 1`: the conductivity is sigmoid(MLP(u)) * kmax) as
ONE ensemble: B members side by side, every launch covering all of them (`odil.util.optimize_ensemble`, traced route).

Member b has its own seed (network initialisation, imposed points), its own weight `kimp` of the imposed points and its
own `kwreg`.  `kimp` reaches the operator as a TRACER of the member's problem: a Python number in the operator is part of
the generated source, and members with different sources run as groups of their own.  `kwreg` is such a number (heat.py
tests it), so the two values swept here give two groups.  The regularisers are annealed with the epoch: the callback
advances `problems[b].tracers["epoch"]`, as the callback of a single run does.

    python examples/heat/ensemble.py --members 64 --Nt 64 --Nx 64 --epochs 200

prints the spread of the inferred k(u) over the members beside `reference_k`, and times the ensemble against the same
members as single `optimize_grad` runs one after the other.
"""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import heat  # noqa: E402

import odil_amd as odil  # noqa: E402
from odil_amd import printlog  # noqa: E402


def operator(ctx):
    """heat.operator with the member's `kimp` read from its tracers (all members then generate one source)."""
    saved = ctx.extra.args
    ctx.extra.args = argparse.Namespace(**{**vars(saved), "kimp": ctx.tracers["kimp"]})
    try:
        return heat.operator(ctx)
    finally:
        ctx.extra.args = saved


def make_members(args):
    """Member b: seed + b (imposed points, network), kimp * (0.5, 1 or 2), kwreg * (1 or 2)."""
    problems, states = [], []
    for b in range(args.members):
        own = argparse.Namespace(**vars(args))
        own.seed = args.seed + b
        own.kwreg = args.kwreg * (1 + b % 2)
        odil.runtime.get_mod().random.set_seed(own.seed)  # (the network's initial weights)
        problem, state = heat.make_problem(own)
        tracers = {"epoch": args.epoch_start, "kimp": args.kimp * 2.0 ** (b % 3 - 1)}
        problems.append(odil.Problem(operator, problem.domain, problem.extra, tracers=tracers))
        states.append(state)
    return problems, states


def conductivity(problem, state, u):
    """The member's k(u) at the temperatures `u` (a NumPy vector)."""
    domain, mod = problem.domain, problem.domain.mod
    net = domain.neural_net(state, "k_net")
    return np.asarray(mod.numpy(mod.sigmoid(net(mod.cast(u, domain.dtype))[0])), dtype=np.float64) * problem.extra.args.kmax


def parse_args(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--Nt", type=int, default=64)
    parser.add_argument("--Nx", type=int, default=64)
    parser.add_argument("--members", type=int, default=16, help="Members of the sweep")
    parser.add_argument("--arch_k", type=int, nargs="*", default=[5, 5], help="Hidden layers of the conductivity net")
    parser.add_argument("--kimp", type=float, default=2, help="Weight of the imposed points (member b: times 0.5, 1 or 2)")
    parser.add_argument("--kwreg", type=float, default=0.05, help="Weight regulariser (member b: times 1 or 2)")
    parser.add_argument("--kwregdecay", type=float, default=50)
    parser.add_argument("--kxreg", type=float, default=0.3)
    parser.add_argument("--kxregdecay", type=float, default=50)
    parser.add_argument("--ktreg", type=float, default=0.2)
    parser.add_argument("--ktregdecay", type=float, default=0)
    parser.add_argument("--nimp", type=int, default=200)
    parser.add_argument("--kmax", type=float, default=0.1)
    parser.add_argument("--single", type=int, default=1, help="Also time the members as single runs")
    parser.add_argument("--repeat", type=int, default=3, help="Timed repetitions of the ensemble and the single runs")
    odil.util.add_arguments(parser)
    parser.set_defaults(outdir="out_heat_ensemble", optimizer="adam", lr=0.001, double=1, multigrid=1, epochs=200,
                        report_every=100, plot_every=0, frames=1)
    args = parser.parse_args(argv)
    args.infer_k, args.imposed, args.keep_frozen, args.keep_init, args.noise = 1, "stripe", 1, 1, 0
    return args


def synchronize():
    import torch

    if torch.cuda.is_available():
        torch.cuda.synchronize()


def main():
    from odil_amd.optimizer import EarlyStopError

    args = parse_args()
    odil.setup_outdir(args)
    if args.optimizer not in ("adam", "lbfgsb"):
        raise SystemExit("--optimizer adam or lbfgsb")
    lbfgsb = args.optimizer == "lbfgsb"
    nsteps = max(args.epochs - args.epoch_start, 1)
    problems, states = make_members(args)
    guess = [[a.clone() for a in problem.domain.arrays_from_state(state)] for problem, state in zip(problems, states)]

    def advance(member, state, epoch, pinfo):
        problems[member].tracers["epoch"] = epoch + 1  # (what the member's next evaluation sees)

    def timed(run):
        for problem, state, arrays in zip(problems, states, guess):
            problem.domain.arrays_to_state([a.clone() for a in arrays], state)
            problem.tracers["epoch"] = args.epoch_start
        synchronize()
        start = time.perf_counter()
        out = run()
        synchronize()
        return 1e3 * (time.perf_counter() - start), out

    def together():
        return odil.util.optimize_ensemble(args, problems, states, advance, form="auto")[1]

    def alone(members=None):
        evals = 0
        for b, (problem, state) in list(enumerate(zip(problems, states)))[:members]:
            callback = lambda state, epoch, pinfo, b=b: advance(b, state, epoch, pinfo)  # noqa: E731
            try:
                evals += odil.util.optimize_grad(args, args.optimizer, problem, state, callback)[1].evals
            except EarlyStopError as stop:  # (L-BFGS-B: a member that converged or gave up before the last epoch)
                evals += stop.optinfo.evals
        return evals

    def report(member, state, epoch, pinfo):
        advance(member, state, epoch, pinfo)
        if epoch % (args.report_every or args.epochs) == 0:
            printlog("epoch={:05d} member {:3d}: loss {:.6e}".format(epoch, member, float(np.array(pinfo["loss"]))))

    _, (arrays, optinfo) = timed(lambda: odil.util.optimize_ensemble(args, problems, states, report, form="auto"))  # (the warm-up)
    ensemble = getattr(optinfo, "ensemble", None)
    lines = ["route '{}', form '{}', {} members in {} group{}".format(
        optinfo.route, optinfo.form, args.members, len(ensemble.groups), "" if len(ensemble.groups) == 1 else "s")]
    u = np.linspace(0.0, 1.0, 6)
    k = np.stack([conductivity(problem, state, u) for problem, state in zip(problems, states)])
    kref = np.asarray(problems[0].domain.mod.numpy(heat.reference_k(problems[0].domain.mod.cast(u, problems[0].domain.dtype),
                                                                     problems[0].domain.mod)))
    lines.append("inferred k(u) over the members after {} epochs: u, min, mean, max | reference_k".format(nsteps))
    for j, uj in enumerate(u):
        lines.append("  u={:.1f}: {:.5f} {:.5f} {:.5f} | {:.5f}".format(uj, k[:, j].min(), k[:, j].mean(), k[:, j].max(), float(kref[j])))
    batches = ensemble.batches
    times, host, rounds = dict(ensemble=[], single=[]), [], []
    if args.single:
        timed(lambda: alone(1))
    for _ in range(max(args.repeat, 1)):
        spent, calls = sum(batch.host_seconds for batch in batches), sum(batch.launches for batch in batches)
        ms, info = timed(together)
        times["ensemble"].append(ms)
        calls = sum(batch.launches for batch in batches) - calls
        # (per epoch of ALL groups: a group's `launch` is counted once per epoch)
        host.append(1e6 * (sum(batch.host_seconds for batch in batches) - spent) / max(calls // len(batches), 1))
        if lbfgsb:
            rounds.append(ms / max(info.rounds, 1))
        if args.single:
            ms, evals = timed(alone)
            times["single"].append((ms, ms / max(evals, 1)))
    span = lambda values: "{:.3f} - {:.3f}".format(min(values), max(values))  # noqa: E731
    if lbfgsb:
        lines.append("ensemble of {} members: {} ms per round of all members ({} rounds, {} repetitions)".format(
            args.members, span(rounds), info.rounds, len(rounds)))
    else:
        lines.append("ensemble of {} members: {} ms per Adam epoch of all members ({} repetitions)".format(
            args.members, span([ms / nsteps for ms in times["ensemble"]]), len(times["ensemble"])))
    lines.append("host time in EpochBatch: {} us per epoch ({} uploads of the argument blocks in all)".format(
        span(host), sum(batch.uploads for batch in batches)))
    if times["single"]:
        ratio = min(ms for ms, _ in times["single"]) / min(times["ensemble"])
        per = "{} ms per evaluation of ONE member".format(span([each for _, each in times["single"]])) if lbfgsb else \
            "{} ms per Adam epoch of all members".format(span([ms / nsteps for ms, _ in times["single"]]))
        lines.append("single runs: {}; all members one after the other take {:.1f} x the ensemble's time{} (best of each)".format(
            per, ratio, "" if ratio >= 1 else ": the ensemble is SLOWER"))
    for line in lines:
        printlog(line)
        if not args.echo:
            print(line)


if __name__ == "__main__":
    main()
