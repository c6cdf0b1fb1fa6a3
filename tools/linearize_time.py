"""Newton steps of `examples/diffusion/ensemble.py` sweeps with all members linearised in one generated launch
(`optimize_newton_ensemble(linearize="batched")`) against member by member (`linearize="members"`, the loop as it was
before the batched Jacobian kernel existed), in one process on one device: per configuration the members are built and both
settings run once (operators traced, kernels loaded), then the two settings alternate, `--reps` repetitions each, from the
same initial guess.  Per-step time: host clock around `--epochs` steps with a synchronise at the end; the linearisation:
device events around it (`optinfo.linearize_ms`).  The iterates of the two settings are compared bit for bit first.

    python tools/linearize_time.py [--reps 3] [--epochs 3] [--configs "256 1 256 0" ...]

--configs: "members ndim N beta" each; default: the five configurations of the README.
Prints one row per configuration: min / median / max per step and the linearisation's share, for both settings.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
import odil_amd as odil  # noqa: E402
import ensemble  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=3)
p.add_argument("--epochs", type=int, default=3)
p.add_argument("--configs", nargs="+", default=["256 1 256 0", "256 2 64 0", "64 3 16 0", "64 3 32 0", "256 2 64 1"])
opt = p.parse_args()
odil.util.set_log_file(open(os.devnull, "w"))


def spread(values):
    return "{:.2f} / {:.2f} / {:.2f}".format(min(values), statistics.median(values), max(values))


print("| members | setting | ms per step (min / median / max of {}) | linearisation ms per step | share of a step | launches per step |".format(opt.reps))
print("|---|---|---|---|---|---|")
for config in opt.configs:
    members, ndim, n, beta = config.split()
    args = ensemble.parse_args("--members {} --ndim {} --N {} --beta {} --kind smooth --linsolver multigrid".format(
        members, ndim, n, beta).split())
    args.epoch_start, args.epochs = 0, opt.epochs
    problems, states = ensemble.make_members(args)
    guess = [problem.domain.arrays_from_state(state)[0].clone() for problem, state in zip(problems, states)]

    def run(how):
        for problem, state, u in zip(problems, states, guess):
            problem.domain.arrays_to_state([u.clone()], state)
        torch.cuda.synchronize()
        start = time.perf_counter()
        arrays, info = odil.util.optimize_newton_ensemble(args, problems, states, linearize=how, time_linearize=True)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - start) / opt.epochs, info, [a[0].clone() for a in arrays]

    first = {how: run(how) for how in ("members", "batched")}  # (also the warm-up)
    same = all(torch.equal(a, b) for a, b in zip(first["members"][2], first["batched"][2]))
    same = same and np.array_equal(first["members"][1].cycles, first["batched"][1].cycles)
    if not same:
        print("| {} | the two settings DIFFER in iterates or cycles |".format(config))
    step, lin, launches = dict(members=[], batched=[]), dict(members=[], batched=[]), dict()
    for _ in range(opt.reps):
        for how in ("members", "batched"):
            ms, info, _ = run(how)
            step[how].append(ms)
            lin[how].append(float(np.mean(info.linearize_ms)))
            launches[how] = int(info.linearize_launches[-1])
    label = "{} x {}{}".format(members, "1-D {}".format(n) if ndim == "1" else "{}^{}".format(n, ndim), ", beta = {}".format(beta) if float(beta) else "")
    for how in ("members", "batched"):
        shares = [100 * l / s for l, s in zip(lin[how], step[how])]
        print("| {} | {} | {} | {} | {:.0f} - {:.0f} % | {} |".format(label, how, spread(step[how]), spread(lin[how]), min(shares),
                                                                     max(shares), launches[how]), flush=True)
