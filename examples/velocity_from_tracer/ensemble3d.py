#!/usr/bin/env python3
"""A sweep of the velocity reconstruction of veltracer3d.py as ONE ensemble: B members on (t, x, y, z) side by side, every
launch covering all four fields (u, vx, vy, vz at 'nccc') of all of them (`odil.util.optimize_ensemble`, traced route; the
transfers run on the rows of [4 B, t, x, y, z] level arrays).

Member b observes its own pair of blobs: the snapshots are shifted with b.  They reach the operator as tensors of the
member's problem, so all members generate one source and run as one group.  `--kxreg_values` optionally sweeps the
Laplacian regularisation weight too: it is a Python number of the operator, hence part of the generated source, and two
values give two groups of members.

    python examples/velocity_from_tracer/ensemble3d.py --members 64 --Nt 8 --Nx 16 --epochs 200

prints the spread of the reconstructed mean velocity over the members, and times the ensemble against the same members as
single `optimize_grad` runs one after the other (alternating in one process after a warm-up: min - max of the repetitions).
"""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import veltracer3d  # noqa: E402

import odil_amd as odil  # noqa: E402
from odil_amd import printlog  # noqa: E402


def make_members(args):
    """Member b: the blobs shifted by b / B of `--shift` in x (first snapshot) and in y (last snapshot); its `kxreg` is
    entry b modulo the count of `--kxreg_values` (default: `--kxreg` for all)."""
    problems, states = [], []
    values = args.kxreg_values or [args.kxreg]
    for b in range(args.members):
        own = argparse.Namespace(**vars(args))
        own.kxreg = values[b % len(values)]
        problem, state = veltracer3d.make_problem(own)
        mod, dtype = problem.domain.mod, problem.domain.dtype
        x, y, z = np.meshgrid(*problem.domain.points_1d("x", "y", "z"), indexing="ij")
        shift = args.shift * b / max(args.members, 1)
        problem.extra.u_init = mod.cast(veltracer3d.blob(x + shift, y, z, 0), dtype)
        problem.extra.u_final = mod.cast(veltracer3d.blob(x, y - shift, z, 1), dtype)
        problems.append(problem)
        states.append(state)
    return problems, states


def mean_velocity(problem, state):
    """(mean vx, mean vy, mean vz) of a member's reconstruction."""
    domain = problem.domain
    return [float(np.mean(np.asarray(domain.mod.numpy(domain.field(state, key)), dtype=np.float64))) for key in veltracer3d.VEL]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--Nt", type=int, default=8)
    parser.add_argument("--Nx", type=int, default=16)
    parser.add_argument("--Ny", type=int, default=None)
    parser.add_argument("--Nz", type=int, default=None)
    parser.add_argument("--members", type=int, default=16, help="Members of the sweep")
    parser.add_argument("--shift", type=float, default=0.1, help="Largest shift of the observed blobs over the members")
    parser.add_argument("--kxreg", type=float, default=0.01, help="Laplacian regularization weight")
    parser.add_argument("--kxreg_values", type=float, nargs="*", default=None,
                        help="Sweep kxreg too: member b takes entry b modulo the count (every value is a group of its own)")
    parser.add_argument("--ktreg", type=float, default=1, help="Time regularization weight")
    parser.add_argument("--kimp", type=float, default=10, help="Imposed values weight")
    parser.add_argument("--single", type=int, default=1, help="Also time the members as single runs")
    parser.add_argument("--repeat", type=int, default=3, help="Timed repetitions of the ensemble and the single runs")
    odil.util.add_arguments(parser)
    odil.linsolver.add_arguments(parser)
    parser.set_defaults(outdir="out_veltracer3d_ensemble", optimizer="adam", lr=0.01, double=1, multigrid=1,
                        epochs=200, report_every=100, plot_every=0, frames=1)
    args = parser.parse_args(argv)
    args.Ny = args.Ny or args.Nx
    args.Nz = args.Nz or args.Nx
    return args


def synchronize():
    import torch

    if torch.cuda.is_available():
        torch.cuda.synchronize()


def main():
    args = parse_args()
    odil.setup_outdir(args)
    if args.optimizer != "adam":
        raise SystemExit("--optimizer adam")
    nsteps = max(args.epochs - args.epoch_start, 1)
    problems, states = make_members(args)
    guess = [[a.clone() for a in problem.domain.arrays_from_state(state)] for problem, state in zip(problems, states)]

    def timed(run):
        for problem, state, arrays in zip(problems, states, guess):
            problem.domain.arrays_to_state([a.clone() for a in arrays], state)
        synchronize()
        start = time.perf_counter()
        out = run()
        synchronize()
        return 1e3 * (time.perf_counter() - start), out

    def together():
        return odil.util.optimize_ensemble(args, problems, states, form="auto")[1]

    def alone(members=None):
        for problem, state in list(zip(problems, states))[:members]:
            odil.util.optimize_grad(args, args.optimizer, problem, state)

    def report(member, state, epoch, pinfo):
        if epoch % (args.report_every or args.epochs) == 0:
            printlog("epoch={:05d} member {:3d}: loss {:.6e}".format(epoch, member, float(np.array(pinfo["loss"]))))

    _, (arrays, optinfo) = timed(lambda: odil.util.optimize_ensemble(args, problems, states, report, form="auto"))  # (the warm-up)
    ensemble = optinfo.ensemble
    lines = ["route '{}', form '{}', {} members x {} fields at '{}' in {} group{}".format(
        optinfo.route, optinfo.form, args.members, ensemble.nfields, ensemble.loc[1:], len(ensemble.groups),
        "" if len(ensemble.groups) == 1 else "s")]
    v = np.array([mean_velocity(problem, state) for problem, state in zip(problems, states)])
    lines.append("mean (vx, vy, vz) over the members after {} epochs: min ({:.4f}, {:.4f}, {:.4f}), max ({:.4f}, {:.4f}, {:.4f})".format(
        nsteps, *v.min(axis=0), *v.max(axis=0)))
    batches = ensemble.batches
    times, host = dict(ensemble=[], single=[]), []
    if args.single:
        timed(lambda: alone(1))
    for _ in range(max(args.repeat, 1)):
        spent, calls = sum(batch.host_seconds for batch in batches), sum(batch.launches for batch in batches)
        ms, _ = timed(together)
        times["ensemble"].append(ms)
        calls = sum(batch.launches for batch in batches) - calls
        # (per epoch of ALL groups: a group's `launch` is counted once per epoch)
        host.append(1e6 * (sum(batch.host_seconds for batch in batches) - spent) / max(calls // len(batches), 1))
        if args.single:
            times["single"].append(timed(alone)[0])
    span = lambda values: "{:.3f} - {:.3f}".format(min(values), max(values))  # noqa: E731
    lines.append("ensemble of {} members: {} ms per Adam epoch of all members ({} repetitions)".format(
        args.members, span([ms / nsteps for ms in times["ensemble"]]), len(times["ensemble"])))
    lines.append("host time in EpochBatch: {} us per epoch ({} uploads of the argument blocks in all)".format(
        span(host), sum(batch.uploads for batch in batches)))
    if times["single"]:
        ratio = min(times["single"]) / min(times["ensemble"])
        lines.append("single runs: {} ms per Adam epoch of all members; all members one after the other take {:.1f} x the "
                     "ensemble's time{} (best of each)".format(span([ms / nsteps for ms in times["single"]]), ratio,
                                                               "" if ratio >= 1 else ": the ensemble is SLOWER"))
    for line in lines:
        printlog(line)
        if not args.echo:
            print(line)


if __name__ == "__main__":
    main()
