"""Time per epoch of ONE ensemble launch (odil_poisson_small_epochs_batch, B members, one workgroup each) against B
back-to-back single-problem launches (odil_poisson_small_epochs) of the same E epochs, in one process on one device:
HIP events around each, a warm-up, then alternating repetitions; min / median / max.

    python tools/ensemble_time.py [--single-lib PATH] [--grid 256] [--levels 8] [--dtype f64] [--epochs 1024]
                                  [--members 1 64 256 512] [--reps 5]

--single-lib: another build of libodil_hip.so whose single-problem entry point is the yardstick (the parent commit's, to
compare against the kernel as it was before the batched form existed); default: this checkout's own.  The members'
results of both sides are compared bit for bit once per B before anything is timed.
--grid: extents of the finest level (1 or 2 numbers); N = 4096 in float64 is the global-memory form.
--form launches: the batched-launch ensemble (fused.PoissonLaunchEnsemble, any 1-D / 2-D size) instead: one epoch of B
members replayed as a hipGraph against B back-to-back replays of a single member's epoch
(PoissonEvaluator.loss_grad_arrays(adam=...), the launches of `optimize_grad`), alternating, each at least --seconds long;
with the bytes an epoch moves (from the shapes) as a share of 8 TB/s.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from odil_amd import _lib, fused, ops  # noqa: E402
from odil_amd.optimizer import _adam_step_size  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--single-lib", default=None)
p.add_argument("--grid", type=int, nargs="+", default=[256])
p.add_argument("--levels", type=int, default=None)
p.add_argument("--dtype", choices=("f64", "f32"), default="f64")
p.add_argument("--epochs", type=int, default=1024)
p.add_argument("--members", type=int, nargs="+", default=[1, 64, 256, 512])
p.add_argument("--reps", type=int, default=5)
p.add_argument("--form", choices=("workgroup", "launches"), default="workgroup")
p.add_argument("--seconds", type=float, default=0.5)
opt = p.parse_args()

dev = torch.device("cuda:0")
dtype = torch.float64 if opt.dtype == "f64" else torch.float32
npdt = np.float64 if opt.dtype == "f64" else np.float32
cshape = tuple(opt.grid)
nlvl = opt.levels or int(round(np.log2(min(cshape))))
shapes = [tuple(n >> l for n in cshape) for l in range(nlvl)]
flat = [n for s in shapes for n in s]
resident = bool(_lib.load().odil_poisson_small_epochs_resident(_lib.i64(flat), nlvl, len(cshape), 8 if opt.dtype == "f64" else 4))
h2 = [npdt(1.0 / n) ** 2 for n in cshape]
E = opt.epochs
table = torch.tensor(np.array([_adam_step_size(npdt(0.005), npdt(0.9), npdt(0.999), npdt(t)) for t in range(1, E + 1)],
                              dtype=np.float64), dtype=dtype, device=dev)
omb1, omb2, eps = float(1 - npdt(0.9)), float(1 - npdt(0.999)), 1e-7

# the yardstick's single-problem entry point
lib = ctypes.CDLL(opt.single_lib) if opt.single_lib else _lib.load()
single = getattr(lib, "odil_poisson_small_epochs_" + opt.dtype)
with open(_lib.HEADER_PATH) as f:
    single.restype, single.argtypes = _lib.declarations(f.read())["odil_poisson_small_epochs_" + opt.dtype]
h2a, h2p = _lib.host_reals(h2, dtype)
shapes_c = _lib.i64(flat)
workspace = ops.reduce_workspace(dev)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def time_launches(B):
    """One row: us per epoch of the ensemble's replayed epoch and of B back-to-back replays of a single member's."""
    gen = torch.Generator().manual_seed(B)
    rhs = torch.randn((B,) + cshape, generator=gen, dtype=torch.float64).to(dtype).to(dev)
    evs = [fused.PoissonEvaluator(cshape, shapes, rhs[b], h2, dtype=dtype, device=dev) for b in range(B)]
    ens = fused.PoissonLaunchEnsemble(evs)
    alpha = table[:1].clone()
    for t in ens.x:
        t.copy_((0.1 * torch.randn(tuple(t.shape), generator=gen, dtype=torch.float64)).to(dtype))
    one = evs[0]
    x1, m1, v1 = ([t[0].clone() for t in arrs] for arrs in (ens.x, ens.m, ens.v))

    def captured(fn):
        fn(), fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph

    g_ens = captured(lambda: ens.epoch(alpha, omb1, omb2, eps))
    g_one = captured(lambda: one.loss_grad_arrays(x1, adam=(m1, v1, alpha, omb1, omb2, eps)))

    def timed(graph, count):
        torch.cuda.synchronize()
        a, b = events()
        a.record()
        for _ in range(count):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / count  # us per replay

    ne = max(4, int(opt.seconds * 1e6 / timed(g_ens, 20)) + 1)
    no = max(4 * B, (int(opt.seconds * 1e6 / timed(g_one, 20)) // B + 1) * B)
    te, ts = [], []
    for _ in range(opt.reps):
        te.append(timed(g_ens, ne))
        ts.append(timed(g_one, no) * B)
    # bytes of an epoch from the shapes: synthesis (read x_l, coarse; write fine), residual (u, rhs, fu), adjoint + update
    # (fu, g, 3 read + 3 written of x, m, v), transposes + updates (read fine g, write g, 6 of x, m, v) per level
    cells = [int(np.prod(s)) for s in shapes]
    words = 3 * cells[0] + 8 * cells[0] + sum(2 * f + c for f, c in zip(cells, cells[1:])) + sum(f + 7 * c for f, c in zip(cells, cells[1:]))
    nbytes = B * words * (8 if opt.dtype == "f64" else 4)
    med = statistics.median(te)
    print(json.dumps(dict(form="launches", members=B, grid=list(cshape), levels=nlvl, dtype=opt.dtype, replays=[ne, no],
                          ensemble_us_per_epoch=[round(f(te), 2) for f in (min, statistics.median, max)],
                          singles_us_per_epoch=[round(f(ts), 2) for f in (min, statistics.median, max)],
                          single_us_per_epoch=round(statistics.median(ts) / B, 2),
                          singles_over_ensemble=round(statistics.median(ts) / med, 2),
                          mbytes_per_epoch=round(nbytes / 1e6, 2), tb_per_s=round(nbytes / med / 1e6, 3),
                          share_of_8_tb_per_s=round(nbytes / med / 1e6 / 8, 3))), flush=True)


if opt.form == "launches":
    print("device:", torch.cuda.get_device_name(0), "| grid", cshape, "levels", nlvl, opt.dtype, "| form: launches", flush=True)
    for B in opt.members:
        time_launches(B)
    sys.exit(0)


print("device:", torch.cuda.get_device_name(0), "| grid", cshape, "levels", nlvl, opt.dtype, "epochs", E,
      "| form:", "LDS-resident" if resident else "global memory", "| single launches from:", opt.single_lib or "this build",
      flush=True)
for B in opt.members:
    gen = torch.Generator().manual_seed(B)
    rhs = torch.randn((B,) + cshape, generator=gen, dtype=torch.float64).to(dtype).to(dev)
    evs = [fused.PoissonEvaluator(cshape, shapes, rhs[b], h2, dtype=dtype, device=dev) for b in range(B)]
    for ev in evs:
        ev.small_force = True
    ens = fused.PoissonEnsemble(evs)
    x0 = (0.1 * torch.randn((B, ens.total), generator=gen, dtype=torch.float64)).to(dtype).to(dev)
    losses, norms = torch.empty((B, E), dtype=dtype, device=dev), torch.empty((B, E), dtype=dtype, device=dev)
    # the single side's own arrays (same layout, separate memory)
    sx, sm, sv, sg, su = (torch.zeros_like(x0) for _ in range(5))
    sfu, sl, sn = torch.empty_like(ens.fu), torch.empty_like(losses), torch.empty_like(norms)
    stream = _lib.stream_ptr()

    def reset():
        ens.x.copy_(x0), ens.m.zero_(), ens.v.zero_()
        sx.copy_(x0), sm.zero_(), sv.zero_()

    def run_ensemble():
        ens.epochs(table, losses, norms, omb1, omb2, eps)

    def run_singles():
        for b in range(B):
            status = single(sx[b].data_ptr(), sm[b].data_ptr(), sv[b].data_ptr(), sg[b].data_ptr(), su[b].data_ptr(),
                            sfu[b].data_ptr(), ens.rhs[b].data_ptr(), shapes_c, nlvl, len(cshape), h2p, table.data_ptr(), E,
                            omb1, omb2, eps, sl[b].data_ptr(), sn[b].data_ptr(), workspace.data_ptr(), stream)
            assert status == 0, status

    def timed(fn):
        reset()
        torch.cuda.synchronize()
        a, b = events()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / E  # us per epoch

    # warm-up, and the results of both sides bit for bit
    reset()
    run_ensemble()
    run_singles()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in ((ens.x, sx), (ens.m, sm), (ens.v, sv), (losses, sl), (norms, sn)))
    te, ts = [], []
    for _ in range(opt.reps):
        te.append(timed(run_ensemble))
        ts.append(timed(run_singles))
    row = dict(members=B, form="resident" if resident else "global", grid=list(cshape), dtype=opt.dtype, epochs=E,
               bit_equal=same,
               ensemble_us_per_epoch=[round(f(te), 2) for f in (min, statistics.median, max)],
               singles_us_per_epoch=[round(f(ts), 2) for f in (min, statistics.median, max)],
               per_member_us_per_epoch=round(statistics.median(te) / B, 3),
               singles_over_ensemble=round(statistics.median(ts) / statistics.median(te), 1))
    print(json.dumps(row), flush=True)
