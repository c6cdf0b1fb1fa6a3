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
    arrays, optinfo = odil.util.optimize_ensemble(args, problems, states, callback, lrs=lrs, form=args.form)
    if args.epochs > args.epoch_start:
        printlog("\nloss at the last epoch, per member:")
        for b, loss in enumerate(optinfo.losses[:, -1].cpu().numpy()):
            printlog("member {:3d}: lr {:.4g} loss {:.6e}".format(b, lrs[b] if lrs else args.lr, float(loss)))


if __name__ == "__main__":
    main()
