#!/usr/bin/env python3
"""An inverse problem on top of examples/diffusion/diffusion.py: infer two constants of

    div((1 + a p) grad u) - s q = 0        (zero walls; p, q given fields)

from noisy observations of u at a random subset of the cells.  The unknowns are the field `u` and `coeff = Array([a, s])`;
the first output is the residual of the equation, the second the weighted data misfit  w mask (u - u_obs).  The data are
made from known constants a*, s*: q is chosen so that the reference solution of diffusion.py solves the discrete equation
with them, and u_obs is that solution plus seeded noise.  (From u = 0 the field has to form before the data can speak:
short runs lower the loss while the constants have hardly moved towards a*, s*.)

Without `--members` it is one `odil.util.optimize` run.  `--members B` sweeps noise seed, initial guess of the constants and
data weight over B members and runs them side by side (`odil.util.optimize_ensemble(form="auto")`: every launch of an epoch
covers all members, the constants of all members are updated by one launch), prints the inferred constants per member and
the time per epoch beside that of the same members as single `optimize_grad` runs one after the other, the two alternating
`--repeat` times after a warm-up.  Everything that differs between members enters the operator as a tensor of `extra`, so
all members generate one kernel source and share their launches.

    python examples/diffusion/infer.py --N 32 --epochs 2000
    python examples/diffusion/infer.py --members 64 --N 64 --epochs 200
    python examples/diffusion/infer.py --members 64 --N 64 --optimizer lbfgsb --epochs 100 --bfgs_m 50
"""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odil_amd as odil  # noqa: E402
from diffusion import conductivity, flux_divergence, reference_solution  # noqa: E402
from odil_amd import printlog  # noqa: E402


def operator(ctx):
    mod, extra = ctx.mod, ctx.extra
    dirs = range(ctx.domain.ndim)
    coeff = ctx.field("coeff")
    st = [ctx.field("u")]
    for i in dirs:
        st.append(ctx.field("u", *[-1 if j == i else 0 for j in dirs]))
        st.append(ctx.field("u", *[1 if j == i else 0 for j in dirs]))
    kfaces = [tuple(1 + coeff[0] * p for p in pair) for pair in extra.pfaces]
    fu = flux_divergence(st, kfaces, dirs, ctx.indices(), ctx.size(), ctx.step(), mod) - coeff[1] * extra.q
    return [("eq", fu), ("data", extra.wmask * (st[0] - extra.u_obs))]


def make_problem(args, seed=None, coeff0=None, weight=None, coeff_first=False):
    """seed: of noise and mask; coeff0: the initial guess of (a, s); weight: w of the data misfit -- default: the
    arguments'.  coeff_first: the `Array` stands before the field in the state."""
    dtype = np.float64 if args.double else np.float32
    ndim = args.ndim
    domain = odil.Domain(cshape=[args.N] * ndim, dimnames=["x", "y", "z"][:ndim], multigrid=args.multigrid, dtype=dtype)
    mod = domain.mod
    x1 = [np.asarray(mod.numpy(x), dtype=np.float64) for x in domain.points_1d()]
    step = [float(s) for s in domain.step()]
    faces = []
    for i in range(ndim):
        pair = []
        for sign in (-0.5, 0.5):
            coords = [x + (sign * step[i] if j == i else 0.0) for j, x in enumerate(x1)]
            pair.append(conductivity("smooth", np.meshgrid(*coords, indexing="ij")) - 1)
        faces.append(tuple(pair))
    pfaces = [tuple(mod.cast(p, dtype) for p in pair) for pair in faces]
    ref = reference_solution(np.meshgrid(*x1, indexing="ij"))
    ref_u = mod.cast(ref, dtype)
    st = [ref_u]
    for i in range(ndim):
        st += [mod.roll(ref_u, 1, i), mod.roll(ref_u, -1, i)]
    ktrue = [tuple(mod.cast(1 + args.a_true * p, dtype) for p in pair) for pair in faces]
    q = flux_divergence(st, ktrue, range(ndim), domain.indices(), domain.size(), domain.step(), mod) / args.s_true
    rng = np.random.default_rng(args.seed if seed is None else seed)
    u_obs = mod.cast(ref + args.noise * rng.standard_normal(ref.shape), dtype)
    mask = rng.random(ref.shape) < args.mask_fraction
    wmask = mod.cast((args.weight if weight is None else weight) * mask, dtype)
    coeff0 = [0.5 * args.a_true, 0.5 * args.s_true] if coeff0 is None else coeff0
    fields = [("coeff", odil.Array(np.asarray(coeff0, dtype=np.float64))), ("u", None)]
    state = odil.State(fields=dict(fields if coeff_first else fields[::-1]))
    state = domain.init_state(state)
    extra = argparse.Namespace(ref_u=ref_u, pfaces=pfaces, q=q, u_obs=u_obs, wmask=wmask, args=args)
    return odil.Problem(operator, domain, extra), state


def constants(problem, state):
    return [float(v) for v in problem.domain.mod.numpy(problem.domain.field(state, "coeff"))]


def make_members(args):
    """Member b: its own noise and mask (seed + b), an initial guess of the constants between 0.5 and 1.5 times the true
    ones, a data weight of w / 2, w or 2 w."""
    built = []
    for b in range(args.members):
        scale = 0.5 + b / max(args.members - 1, 1)
        built.append(make_problem(args, seed=args.seed + b, coeff0=[scale * args.a_true, scale * args.s_true],
                                  weight=args.weight * 2.0 ** (b % 3 - 1)))
    return [p for p, _ in built], [s for _, s in built]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--ndim", type=int, choices=[1, 2, 3], default=2, help="Space dimension")
    parser.add_argument("--N", type=int, default=32, help="Grid size")
    parser.add_argument("--a_true", type=float, default=1.0, help="a*: amplitude of the conductivity 1 + a p")
    parser.add_argument("--s_true", type=float, default=2.0, help="s*: strength of the source s q")
    parser.add_argument("--noise", type=float, default=0.01, help="Standard deviation of the noise on the observations")
    parser.add_argument("--mask_fraction", type=float, default=0.25, help="Share of the cells that are observed")
    parser.add_argument("--weight", type=float, default=1.0, help="w: weight of the data misfit")
    # (--seed, of `odil.util.add_arguments`: of noise and mask; member b: seed + b)
    parser.add_argument("--members", type=int, default=0, help="Sweep this many members side by side (0: one plain run)")
    parser.add_argument("--single", type=int, default=1, help="--members: also time the members as single runs")
    parser.add_argument("--repeat", type=int, default=3, help="--members: timed repetitions of the ensemble and the single runs")
    odil.util.add_arguments(parser)
    parser.set_defaults(frames=1, report_every=100, history_every=10, plot_every=0, history_full=50)
    parser.set_defaults(optimizer="adam", multigrid=1, lr=0.005, double=1, outdir="out_diffusion_infer", epochs=1000)
    return parser.parse_args(argv)


def synchronize():
    import torch

    if torch.cuda.is_available():
        torch.cuda.synchronize()


def main_members(args):
    """The sweep: all members per launch against the same members one after the other."""
    from odil_amd.optimizer import EarlyStopError

    nsteps = max(args.epochs - args.epoch_start, 1)
    lbfgsb = args.optimizer == "lbfgsb"
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
        evals = 0
        for problem, state in list(zip(problems, states))[:members]:
            try:
                evals += odil.util.optimize_grad(args, args.optimizer, problem, state)[1].evals
            except EarlyStopError as stop:  # (L-BFGS-B: a member that converged or gave up before the last epoch)
                evals += stop.optinfo.evals
        return evals

    def callback(member, state, epoch, pinfo):
        if member == 0:
            printlog("\nepoch={:05d}".format(epoch))
        printlog("member {:3d}: loss {:.6e}, a={:.5g}, s={:.5g}".format(
            member, float(np.array(pinfo["loss"])), *constants(problems[member], state)))

    every = args.report_every or args.epochs
    callback.next_active = lambda epoch: (epoch // every + 1) * every
    arrays, optinfo = odil.util.optimize_ensemble(args, problems, states, callback, form="auto")  # (the warm-up, with the report)
    lines = ["route '{}', form '{}', true constants a={:.5g}, s={:.5g}".format(optinfo.route, optinfo.form, args.a_true, args.s_true)]
    for b, (problem, state) in enumerate(zip(problems, states)):
        lines.append("member {:3d}: a={:.5g}, s={:.5g}".format(b, *constants(problem, state)))
    batches = getattr(getattr(optinfo, "ensemble", None), "batches", [])
    times, host, reads, rounds = dict(ensemble=[], single=[]), [], [], []
    if args.single:
        timed(lambda: alone(1))
    for _ in range(max(args.repeat, 1) if args.epochs > args.epoch_start else 0):
        spent, calls = sum(batch.host_seconds for batch in batches), sum(batch.launches for batch in batches)
        ms, info = timed(together)
        times["ensemble"].append(ms)
        calls = sum(batch.launches for batch in batches) - calls
        host.append(1e6 * (sum(batch.host_seconds for batch in batches) - spent) / max(calls, 1))
        if lbfgsb:
            rounds.append(ms / max(info.rounds, 1))
            reads.append(1e3 * info.read_seconds / max(info.rounds, 1))
        if args.single:
            ms, evals = timed(alone)
            times["single"].append((ms, ms / max(evals, 1)))
    span = lambda values: "{:.3f} - {:.3f}".format(min(values), max(values))
    if times["ensemble"] and lbfgsb:
        lines.append("ensemble of {} members: {} ms per round of all members ({} rounds, {} repetitions), of which the host is "
                     "blocked in the two reads for {} ms".format(args.members, span(rounds), optinfo.rounds, len(rounds), span(reads)))
    elif times["ensemble"]:
        lines.append("ensemble of {} members: {} ms per Adam epoch of all members ({} repetitions)".format(
            args.members, span([ms / nsteps for ms in times["ensemble"]]), len(times["ensemble"])))
    if times["ensemble"] and batches:
        lines.append("host time in EpochBatch: {} us per call".format(span(host)))
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


def main():
    args = parse_args()
    odil.setup_outdir(args)
    if args.members:
        return main_members(args)
    problem, state = make_problem(args)

    def history_func(p, s, epoch, history, cbinfo):
        for name, v in zip(("a", "s"), constants(p, s)):
            history.append(name, v)

    callback = odil.make_callback(
        problem, args, history_func=history_func,
        report_func=lambda p, s, epoch, cbinfo: printlog("a={:.5g} (true {:.5g}), s={:.5g} (true {:.5g})".format(
            constants(p, s)[0], args.a_true, constants(p, s)[1], args.s_true)))
    odil.optimize(args, args.optimizer, problem, state, callback)


if __name__ == "__main__":
    main()
