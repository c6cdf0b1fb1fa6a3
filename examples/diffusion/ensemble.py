#!/usr/bin/env python3
"""A sweep over the conductivity of examples/diffusion/diffusion.py solved side by side: B members with the conductivity
1 + a_b (k - 1), the amplitude a_b running from 1 / B to 1 over the members, every Newton step of all members in ONE
solve launch, one workgroup per member (`odil.util.optimize_newton_ensemble`, its route for variable-coefficient
stencils).  With `--beta > 0` the operator is nonlinear,  div(k grad u) - beta u^3 = f,  and the members' multigrid
hierarchies are set up again every step.  Every step linearises all members in one generated launch (`--linearize
batched`, `odil.util.linearize_ensemble`) or member by member (`--linearize members`); the linearisation's share of a step
is printed from device events around it.  The time per step is printed beside that of the same members as single
`optimize_newton` runs, one after the other (`--single 0` skips those).  `--form launches` runs members that are too large
for one workgroup (256^2, 64^3, 128^3): the levels above 32768 cells as launches that cover all members, the convergence
decision on the device (`gmg.EnsembleLaunchGMG`); `--form auto` takes it only where `--form workgroup` refuses.
`--pair_min_cells N` sets from how many cells of all members together a launch level smooths twice per pass
(`odil_stencil_var_smooth2_batch`; 0: always, -1: never).
`--velocity V` adds first-order upwind convection,  div(k grad u) - v du/dx_0 - beta u^3 = f  with v_b = V (b + 1) / B
(`--velocity_from V0`: v_b = V0 + (V - V0) (b + 1) / B) swept over the members like the conductivity amplitude (the Jacobian stays a (2 d + 1)-point stencil); the members of an
ensemble walk one set of levels, so V is chosen where they coarsen alike (e.g. `--N 8 --ndim 3 --velocity 800 --members 4`:
v = 200 ... 800), and a refusal is printed as it is.  `--krylov auto` hands a member whose cycles stop contracting to GCR(6)
inside the solve launch (`optimize_newton_ensemble(krylov="auto")`); `--krylov any` does so in whichever form runs the
members, with `--form launches` across the batched launches (`gmg.EnsembleLaunchKrylovGMG`); `--krylov never` reports it as
not converged.
`--alternate R` times the ensemble and the single runs R more times, alternating in one process, and prints min - max.

`--optimizer adam` runs the same sweep with Adam (`odil.util.optimize_ensemble(form="auto")`, its route for traced stencil
operators: every launch of an epoch covers all members; `--multigrid 1` for a multigrid-decomposed unknown) and prints the
time per epoch of all members beside that of the same members as single `optimize_grad` runs one after the other, the two
alternating `--repeat` times, with the host time `stencil_bind.EpochBatch` spends per epoch.

    python examples/diffusion/ensemble.py --members 64 --ndim 2 --N 64 --kind smooth --epochs 2
    python examples/diffusion/ensemble.py --members 64 --ndim 2 --N 64 --beta 1 --epochs 4
    python examples/diffusion/ensemble.py --members 256 --ndim 2 --N 64 --linearize members --single 0
    python examples/diffusion/ensemble.py --members 16 --ndim 2 --N 256 --form launches --linsolver multigrid
    python examples/diffusion/ensemble.py --members 64 --ndim 2 --N 64 --optimizer adam --multigrid 1 --epochs 200

`--optimizer lbfgsb` runs it with L-BFGS-B, all members in lock-step: a round is one evaluation of all members, the batched
vector launches and two host reads.  Printed: the time per round of all members and the host time blocked in the reads,
beside the time per evaluation of the same members as single `optimize_grad(args, "lbfgsb", ...)` runs one after the other.

    python examples/diffusion/ensemble.py --members 64 --ndim 2 --N 64 --optimizer lbfgsb --multigrid 1 --epochs 100
"""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odil_amd as odil  # noqa: E402
import diffusion  # noqa: E402
from odil_amd import printlog  # noqa: E402


def operator(ctx):
    """div(k grad u) - beta u^3 - rhs on top of diffusion.flux_divergence (beta = 0: diffusion.operator)."""
    mod, extra = ctx.mod, ctx.extra
    dirs = range(ctx.domain.ndim)
    st = [ctx.field("u")]
    for i in dirs:
        st.append(ctx.field("u", *[-1 if j == i else 0 for j in dirs]))
        st.append(ctx.field("u", *[1 if j == i else 0 for j in dirs]))
    fu = diffusion.flux_divergence(st, extra.kfaces, dirs, ctx.indices(), ctx.size(), ctx.step(), mod, extra.args.sigma)
    if getattr(extra, "velocity", 0.0):
        fu = fu - upwind_convection(st[0], st[1], extra.velocity, ctx.indices(), ctx.size(), ctx.step(), mod)
    if extra.beta:
        fu = fu - extra.beta * (st[0] * st[0] * st[0])
    return [fu - extra.rhs]


def upwind_convection(q, qm, velocity, iw, nw, dw, mod):
    """v du/dx_0 by first-order upwinding (v > 0: the difference towards -e_0) on the rows away from the walls of axis 0."""
    zero = mod.cast(0, q.dtype)
    inner = velocity * (q - qm) / dw[0]
    return mod.where(iw[0] == 0, zero, mod.where(iw[0] == nw[0] - 1, zero, inner))


def parse_args(argv=None):
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument("--members", type=int, default=16, help="Problems in the ensemble")
    own.add_argument("--beta", type=float, default=0.0, help="Strength of the nonlinear term: div(k grad u) - beta u^3 = f")
    own.add_argument("--single", type=int, default=1, help="Also run the members as single optimize_newton runs and time them")
    own.add_argument("--linearize", type=str, default="batched", choices=("batched", "members"),
                     help="Linearise all members in one generated launch, or member by member")
    own.add_argument("--form", type=str, default="workgroup", choices=("workgroup", "launches", "auto"),
                     help="One workgroup per member, batched launches for members beyond one workgroup, or whichever serves")
    own.add_argument("--pair_min_cells", type=int, default=None,
                     help="--form launches: levels on which all members together have at least N cells smooth twice per pass "
                          "(gmg.EnsembleLaunchGMG.pair_min_cells; 0: always, -1: never; default: the class's)")
    own.add_argument("--velocity", type=float, default=0.0,
                     help="Upwind convection - v du/dx_0, v swept over the members up to this value (0: none)")
    own.add_argument("--velocity_from", type=float, default=0.0,
                     help="The sweep of v starts above this value: v_b = from + (V - from) (b + 1) / B")
    own.add_argument("--krylov", type=str, default="never", choices=("never", "auto", "any"),
                     help="Newton: hand a member whose cycles stop contracting to GCR inside the solve launch (auto: --form "
                          "workgroup only) or in whichever form runs the members (any: also across the batched launches)")
    own.add_argument("--alternate", type=int, default=0,
                     help="Newton: after the report, time the ensemble and the single runs alternating this many times")
    own.add_argument("--repeat", type=int, default=3, help="--optimizer adam: timed repetitions of the ensemble and the single runs")
    mine, rest = own.parse_known_args(argv)
    args = diffusion.parse_args(["--ndim", "2", "--N", "16", "--epochs", "2"] + rest)
    for key, value in vars(mine).items():
        setattr(args, key, value)
    return args


def make_member(args, b):
    """Member b: conductivity 1 + a_b (k - 1), a_b = (b + 1) / members; the right-hand side is the discrete operator of
    that member on the reference solution, so every member has the same solution."""
    problem, state = diffusion.make_problem(args)
    domain, extra = problem.domain, problem.extra
    mod = domain.mod
    amp = (b + 1) / args.members
    extra.kfaces = [tuple(1 + amp * (k - 1) for k in pair) for pair in extra.kfaces]
    extra.beta = float(args.beta)
    lowest = float(getattr(args, "velocity_from", 0.0))
    extra.velocity = lowest + (float(getattr(args, "velocity", 0.0)) - lowest) * amp if getattr(args, "velocity", 0.0) else 0.0
    ndim = domain.ndim
    st = [extra.ref_u]
    for i in range(ndim):
        st += [mod.roll(extra.ref_u, 1, i), mod.roll(extra.ref_u, -1, i)]
    extra.rhs = diffusion.flux_divergence(st, extra.kfaces, range(ndim), domain.indices(), domain.size(), domain.step(), mod,
                                          args.sigma)
    if extra.velocity:
        extra.rhs = extra.rhs - upwind_convection(st[0], st[1], extra.velocity, domain.indices(), domain.size(), domain.step(), mod)
    if args.beta:
        extra.rhs = extra.rhs - extra.beta * (extra.ref_u * extra.ref_u * extra.ref_u)
    return odil.Problem(operator, domain, extra), state


def make_members(args):
    built = [make_member(args, b) for b in range(args.members)]
    return [p for p, _ in built], [s for _, s in built]


def synchronize():
    import torch

    if torch.cuda.is_available():
        torch.cuda.synchronize()


def main_adam(args, callback):
    """The sweep with Adam: all members per launch against the same members one after the other."""
    nsteps = max(args.epochs - args.epoch_start, 1)
    problems, states = make_members(args)
    guess = [[a.clone() for a in problem.domain.arrays_from_state(state)] for problem, state in zip(problems, states)]

    def restart():
        for problem, state, arrays in zip(problems, states, guess):
            problem.domain.arrays_to_state([a.clone() for a in arrays], state)
        synchronize()

    def timed(run):
        restart()
        start = time.perf_counter()
        run()
        synchronize()
        return 1e3 * (time.perf_counter() - start) / nsteps

    def together():
        return odil.util.optimize_ensemble(args, problems, states, form="auto")

    def alone():
        for problem, state in zip(problems, states):
            odil.util.optimize_grad(args, "adam", problem, state)

    # the warm-up: every operator traced, every kernel of both routes loaded, the report of the sweep
    arrays, optinfo = odil.util.optimize_ensemble(args, problems, states, callback, form="auto")
    printlog("\nroute '{}', form '{}'".format(optinfo.route, optinfo.form))
    for b, (problem, state) in enumerate(zip(problems, states)):
        printlog("member {:3d}: loss {:.6e}, error u:{:.5g}".format(
            b, float(optinfo.losses[b, -1]) if nsteps and optinfo.losses.numel() else float("nan"),
            diffusion.error_rms(problem.domain, problem.extra, state, "u")))
    batches = getattr(getattr(optinfo, "ensemble", None), "batches", [])
    times, host = dict(ensemble=[], single=[]), []
    if args.single:
        timed(lambda: odil.util.optimize_grad(args, "adam", problems[0], states[0]))
    for _ in range(max(args.repeat, 1) if args.epochs > args.epoch_start else 0):
        spent, calls = sum(batch.host_seconds for batch in batches), sum(batch.launches for batch in batches)
        times["ensemble"].append(timed(together))
        calls = sum(batch.launches for batch in batches) - calls
        host.append((1e6 * (sum(batch.host_seconds for batch in batches) - spent) / max(calls, 1), calls))
        if args.single:
            times["single"].append(timed(alone))
    span = lambda values: "{:.3f} - {:.3f}".format(min(values), max(values))
    lines = []
    if times["ensemble"]:
        lines.append("ensemble of {} members: {} ms per Adam epoch of all members ({} repetitions)".format(
            args.members, span(times["ensemble"]), len(times["ensemble"])))
        if batches:
            # (epochs replayed as a graph make no call: the launches were captured once)
            lines.append("host time in EpochBatch: {} us per call, {} calls in {} epochs (the argument blocks uploaded {} "
                         "times in all)".format(span([us for us, _ in host]), host[-1][1], nsteps,
                                                sum(batch.uploads for batch in batches)))
    if times["single"]:
        lines.append("single runs: {} ms per Adam epoch of all members, {:.1f} x the ensemble (best of each)".format(
            span(times["single"]), min(times["single"]) / min(times["ensemble"])))
    for line in lines:
        printlog(line)
        if not args.echo:
            print(line)


def main_lbfgsb(args, callback):
    """The sweep with L-BFGS-B: all members in lock-step (`odil.util.optimize_ensemble`, one evaluation of all members per
    round) against the same members as single `optimize_grad` runs one after the other, the two alternating `--repeat`
    times after a warm-up."""
    from odil_amd.optimizer import EarlyStopError

    problems, states = make_members(args)
    guess = [[a.clone() for a in problem.domain.arrays_from_state(state)] for problem, state in zip(problems, states)]

    def restart():
        for problem, state, arrays in zip(problems, states, guess):
            problem.domain.arrays_to_state([a.clone() for a in arrays], state)
        synchronize()

    def timed(run):
        restart()
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
                evals += odil.util.optimize_grad(args, "lbfgsb", problem, state)[1].evals
            except EarlyStopError as stop:  # (a member that converged or gave up before the last epoch)
                evals += stop.optinfo.evals
        return evals

    arrays, optinfo = odil.util.optimize_ensemble(args, problems, states, callback, form="auto")  # (the warm-up, with the report)
    printlog("\nroute '{}', form '{}', {} rounds, {} host reads".format(optinfo.route, optinfo.form, optinfo.rounds, optinfo.host_reads))
    for b, (problem, state) in enumerate(zip(problems, states)):
        printlog("member {:3d}: {} iterations, {} evaluations, {}; error u:{:.5g}".format(
            b, optinfo.nits[b], optinfo.evals[b], optinfo.tasks[b], diffusion.error_rms(problem.domain, problem.extra, state, "u")))
    if args.single:
        timed(lambda: alone(1))
    rounds, reads, total, singles = [], [], [], []
    for _ in range(max(args.repeat, 1) if args.epochs > args.epoch_start else 0):
        ms, info = timed(together)
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
    nsteps = max(args.epochs - args.epoch_start, 1)

    def callback(member, state, epoch, pinfo):
        if member == 0:
            printlog("\nepoch={:05d}".format(epoch))
        printlog("member {:3d}: loss {:.6e}".format(member, float(np.array(pinfo["loss"]))))

    every = args.report_every or args.epochs
    callback.next_active = lambda epoch: (epoch // every + 1) * every
    if args.optimizer in ("adam", "adamn"):
        return main_adam(args, callback)
    if args.optimizer == "lbfgsb":
        return main_lbfgsb(args, callback)
    if args.pair_min_cells is not None:  # (for this run: the driver builds its solver from the class)
        from odil_amd import gmg

        gmg.EnsembleLaunchGMG.pair_min_cells = float("inf") if args.pair_min_cells < 0 else args.pair_min_cells
    problems, states = make_members(args)
    guess = [problem.domain.arrays_from_state(state)[0].clone() for problem, state in zip(problems, states)]

    def restart():
        for problem, state, u in zip(problems, states, guess):
            problem.domain.arrays_to_state([u.clone()], state)
        synchronize()

    try:
        arrays, optinfo = odil.util.optimize_newton_ensemble(args, problems, states, callback, linearize=args.linearize,
                                                               form=args.form, krylov=args.krylov)
    except ValueError as refusal:
        if not (args.velocity or args.krylov != "never"):
            raise  # (command lines without the two options: as before)
        print(refusal)  # (members that coarsen differently, a form that has no hand-over, ...: as it is)
        raise SystemExit(1)
    import torch

    together, timed = None, optinfo.route == "stencil" and torch.cuda.is_available()
    if args.epochs > args.epoch_start:  # (the same steps again, now that every member's operator is traced and its kernels are loaded)
        restart()
        start = time.perf_counter()
        arrays, optinfo = odil.util.optimize_newton_ensemble(args, problems, states, linearize=args.linearize, time_linearize=timed,
                                                               form=args.form, krylov=args.krylov)
        synchronize()
        together = (time.perf_counter() - start) / nsteps
    status = [optinfo.solver.status(b) for b in range(args.members)] if optinfo.solver is not None else []
    printlog("\nroute '{}', form '{}', last Newton step, per member:".format(optinfo.route, optinfo.form))
    for b, (problem, state, st) in enumerate(zip(problems, states, status)):
        handed = "" if st.get("handover") is None else ", handed to GCR before cycle {}".format(st["handover"])
        printlog("member {:3d}: {} cycles{}, relative residual {:.2e}{}, error u:{:.5g}".format(
            b, st["niter"], handed, st["residual"] / max(st["bnorm"], 1e-300), "" if st["converged"] else " (not converged)",
            diffusion.error_rms(problem.domain, problem.extra, state, "u")))
    lines = ["{} converged members of {}".format(sum(bool(st["converged"]) for st in status), args.members)]
    if args.krylov != "never":
        handed = [int(st["handover"]) for st in status if st.get("handover") is not None]
        lines.append("{} members handed to GCR {}{}".format(
            len(handed), "inside the launch" if optinfo.form == "workgroup" else "across the launches", " (before cycles {} ... {})".format(min(handed), max(handed)) if handed else ""))
    if status and (args.velocity or args.krylov != "never"):
        lines.append("passes per member: {} ... {}".format(min(st["niter"] for st in status), max(st["niter"] for st in status)))
    if together is not None:
        lines.append("ensemble: {:.3f} ms per Newton step of all members".format(1e3 * together))
    if together is not None and optinfo.linearize_ms is not None:
        share = float(np.mean(optinfo.linearize_ms))
        lines.append("linearisation ({}, {} launches per step): {:.3f} ms per step, {:.0f} % of a step".format(
            args.linearize, int(optinfo.linearize_launches[-1]), share, 100 * share / (1e3 * together)))
    if args.single and together is not None:
        restart()
        odil.util.optimize_newton(args, problems[0], states[0])  # (the kernels of the single route, loaded once)
        restart()
        start = time.perf_counter()
        for problem, state in zip(problems, states):
            odil.util.optimize_newton(args, problem, state)
        synchronize()
        alone = (time.perf_counter() - start) / nsteps
        lines.append("single runs: {:.3f} ms per Newton step of all members, {:.1f} x the ensemble".format(
            1e3 * alone, alone / together))
    if args.alternate > 0 and together is not None:
        # every kernel of both routes is loaded by now (a single run that hands over to GCR loads its own on the way)
        def ensemble_steps():
            odil.util.optimize_newton_ensemble(args, problems, states, linearize=args.linearize, form=args.form, krylov=args.krylov)

        def single_steps():
            for problem, state in zip(problems, states):
                odil.util.optimize_newton(args, problem, state)

        times = dict(ensemble=[], single=[])
        for _ in range(args.alternate):
            for name, run in (("ensemble", ensemble_steps), ("single", single_steps)):
                if name == "single" and not args.single:
                    continue
                restart()
                start = time.perf_counter()
                run()
                synchronize()
                times[name].append(1e3 * (time.perf_counter() - start) / nsteps)
        span = lambda values: "{:.3f} - {:.3f}".format(min(values), max(values))
        lines.append("alternating, {} repetitions: ensemble {} ms per Newton step of all members".format(
            args.alternate, span(times["ensemble"])))
        if times["single"]:
            lines.append("alternating: single runs {} ms per Newton step of all members, {:.1f} x the ensemble (best of "
                         "each)".format(span(times["single"]), min(times["single"]) / min(times["ensemble"])))
    for line in lines:
        printlog(line)
        if not args.echo:  # (the log goes to train.log: the verdict also to the terminal)
            print(line)


if __name__ == "__main__":
    main()
