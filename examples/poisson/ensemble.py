#!/usr/bin/env python3
"""A sweep of small Poisson problems solved side by side: B members of examples/poisson/poisson.py that differ by their
right-hand side (`--vary rhs`: the reference solution scaled and noise added to the imposed data) or by their initial
guess (`--vary guess`), all in ONE launch per chunk of epochs, one workgroup per member (`odil.util.optimize_ensemble`).
Alone, a problem of this size uses one of the device's 256 compute units.  Larger members (2-D N = 64 ... 256, long 1-D
grids) run with `--form launches`: the launches of a single run's epoch, each covering all members; 3-D members run the
same way with `--form volumes` (or `--form auto`, which picks the form from the members' shapes).

    python examples/poisson/ensemble.py --ndim 1 --N 256 --members 64 --epochs 1000 --vary rhs
    python examples/poisson/ensemble.py --ndim 2 --N 128 --members 64 --epochs 1000 --form launches
    python examples/poisson/ensemble.py --ndim 3 --N 32 --members 64 --epochs 1000 --form volumes

With `--optimizer newton` (plain unknowns, `--multigrid 0`) every epoch is ONE launch that runs the whole Newton step of
every member, one workgroup per member (`odil.util.optimize_newton_ensemble`):

    python examples/poisson/ensemble.py --ndim 3 --N 16 --members 64 --multigrid 0 --optimizer newton --linsolver multigrid --epochs 1

Members beyond one workgroup (256^2, 64^3) take `--form launches` there too (or `--form auto`): the stencil route of the
Newton driver with the large levels as launches that cover all members (`gmg.EnsembleLaunchGMG`):

    python examples/poisson/ensemble.py --ndim 2 --N 256 --members 16 --multigrid 0 --optimizer newton --linsolver multigrid --epochs 1 --form launches

With `--optimizer lbfgsb` all members run L-BFGS-B in lock-step as batched launches (a round: one evaluation of all
members, the batched vector algebra, two host reads), timed beside the same members as single runs:

    python examples/poisson/ensemble.py --ndim 2 --N 64 --members 64 --optimizer lbfgsb --epochs 100 --form auto
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odil_amd as odil  # noqa: E402
import poisson  # noqa: E402
from odil_amd import printlog  # noqa: E402


def parse_args(argv=None):
    import argparse

    own = argparse.ArgumentParser(add_help=False)
    own.add_argument("--members", type=int, default=16, help="Problems in the ensemble")
    own.add_argument("--vary", choices=("rhs", "guess"), default="rhs", help="What differs between the members")
    own.add_argument("--noise", type=float, default=0.1, help="Amplitude of the noise on the right-hand side / the guess")
    own.add_argument("--lr_spread", type=float, default=1.0, help="Step sizes from lr / spread to lr * spread over the members")
    own.add_argument("--form", choices=("workgroup", "launches", "volumes", "auto"), default="workgroup",
                     help="One workgroup per member (small members), batched launches (any 1-D / 2-D size), batched launches "
                          "of 3-D members, or whichever fits")
    own.add_argument("--single", type=int, default=1, help="--optimizer lbfgsb: also time the members as single runs")
    own.add_argument("--repeat", type=int, default=3, help="--optimizer lbfgsb: timed repetitions of the ensemble and the single runs")
    mine, rest = own.parse_known_args(argv)
    args = poisson.parse_args(["--ndim", "1", "--N", "256"] + rest)
    for key, value in vars(mine).items():
        setattr(args, key, value)
    return args


def make_members(args):
    rng = np.random.default_rng(args.seed or 0)
    problems, states = [], []
    for b in range(args.members):
        problem, state = poisson.make_problem(args)
        domain = problem.domain
        if args.vary == "rhs":
            noise = domain.mod.array(rng.standard_normal(domain.cshape).astype(domain.dtype))
            problem.extra.rhs = problem.extra.rhs * (1 + b / args.members) + args.noise * noise
        else:
            arrays = domain.arrays_from_state(state)
            arrays[0] = domain.mod.array((args.noise * rng.standard_normal(tuple(arrays[0].shape))).astype(domain.dtype))
            domain.arrays_to_state(arrays, state)
        problems.append(problem)
        states.append(state)
    return problems, states


def main_lbfgsb(args, problems, states, callback):
    """The sweep with L-BFGS-B, all members in lock-step (a round: one evaluation of all members, the batched vector
    launches, two host reads), timed against the same members as single `optimize_grad` runs one after the other; the two
    alternate `--repeat` times after a warm-up."""
    import time

    import torch

    from odil_amd.optimizer import EarlyStopError

    form = "auto" if args.form == "workgroup" else args.form  # (the one-workgroup epochs are Adam's)
    guess = [[a.clone() for a in problem.domain.arrays_from_state(state)] for problem, state in zip(problems, states)]

    def timed(run):
        for problem, state, arrays in zip(problems, states, guess):
            problem.domain.arrays_to_state([a.clone() for a in arrays], state)
        torch.cuda.synchronize()
        start = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - start), out

    def alone(members=None):
        evals = 0
        for problem, state in list(zip(problems, states))[:members]:
            try:
                evals += odil.util.optimize_grad(args, "lbfgsb", problem, state)[1].evals
            except EarlyStopError as stop:  # (a member that converged or gave up before the last epoch)
                evals += stop.optinfo.evals
        return evals

    arrays, optinfo = odil.util.optimize_ensemble(args, problems, states, callback, form=form)  # (warm-up and report)
    printlog("\nroute '{}', form '{}', {} rounds, {} host reads".format(optinfo.route, optinfo.form, optinfo.rounds, optinfo.host_reads))
    for b in range(args.members):
        printlog("member {:3d}: {} iterations, {} evaluations, {}".format(b, optinfo.nits[b], optinfo.evals[b], optinfo.tasks[b]))
    if args.single:
        timed(lambda: alone(1))
    rounds, reads, total, singles = [], [], [], []
    for _ in range(max(args.repeat, 1) if args.epochs > args.epoch_start else 0):
        ms, info = timed(lambda: odil.util.optimize_ensemble(args, problems, states, form=form)[1])
        total.append(ms)
        rounds.append(ms / max(info.rounds, 1))
        reads.append(1e3 * info.read_seconds / max(info.rounds, 1))
        if args.single:
            ms, evals = timed(alone)
            singles.append((ms, ms / max(evals, 1)))
    span = lambda values: "{:.3f} - {:.3f}".format(min(values), max(values))
    lines = []
    if rounds:
        lines.append("ensemble of {} members: {} ms per round of all members ({} rounds, {} repetitions), of which the host "
                     "is blocked in the two reads for {} ms".format(args.members, span(rounds), optinfo.rounds, len(rounds), span(reads)))
    if singles:
        ratio = min(ms for ms, _ in singles) / min(total)
        lines.append("single runs: {} ms per evaluation of ONE member; all members one after the other take {:.1f} x the "
                     "ensemble's time{} (best of each)".format(span([each for _, each in singles]), ratio,
                                                              "" if ratio >= 1 else ": the ensemble is SLOWER"))
    for line in lines:
        printlog(line)
        if not args.echo:
            print(line)


def main():
    args = parse_args()
    odil.setup_outdir(args)
    problems, states = make_members(args)
    lrs = None
    if args.lr_spread != 1.0:
        lrs = list(args.lr * np.geomspace(1 / args.lr_spread, args.lr_spread, args.members))

    def callback(member, state, epoch, pinfo):
        if member == 0:
            printlog("\nepoch={:05d}".format(epoch))
        printlog("member {:3d}: loss {:.6e}".format(member, float(np.array(pinfo["loss"]))))

    every = args.report_every or args.epochs
    callback.next_active = lambda epoch: (epoch // every + 1) * every
    if args.optimizer == "newton":
        # one launch per epoch runs the whole Newton step of every member (one workgroup per member)
        arrays, optinfo = odil.util.optimize_newton_ensemble(args, problems, states, callback, form=args.form)
        if args.epochs > args.epoch_start:
            status = [optinfo.solver.status(b) for b in range(args.members)]
            printlog("\nlast Newton step, per member:")
            for b, st in enumerate(status):
                printlog("member {:3d}: {} cycles, relative residual {:.2e}{}".format(
                    b, st["niter"], st["residual"] / max(st["bnorm"], 1e-300), "" if st["converged"] else " (not converged)"))
            summary = "{} converged members of {}".format(sum(bool(st["converged"]) for st in status), args.members)
            printlog(summary)
            if not args.echo:  # (the log goes to train.log: the verdict also to the terminal)
                print(summary)
        return
    if args.optimizer == "lbfgsb":
        return main_lbfgsb(args, problems, states, callback)
    arrays, optinfo = odil.util.optimize_ensemble(args, problems, states, callback, lrs=lrs, form=args.form)
    if args.epochs > args.epoch_start:
        printlog("\nloss at the last epoch, per member:")
        for b, loss in enumerate(optinfo.losses[:, -1].cpu().numpy()):
            printlog("member {:3d}: lr {:.4g} loss {:.6e}".format(b, lrs[b] if lrs else args.lr, float(loss)))


if __name__ == "__main__":
    main()
