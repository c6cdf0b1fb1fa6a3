#!/usr/bin/env python3
"""Headline benchmark: grid-point-updates/s of the ODIL hot path on MI355X.

Default workload (BASELINE.json metric, config "4a"): 3-D Poisson 512^3, multigrid decomposition (9 levels),
f64, Adam -- one "step" is one optimizer epoch of the reference's hot loop
(reference src/odil/optimizer.py:331-336): multigrid synthesis -> residual + loss ->
adjoint -> P^T chain -> Adam update.  Metric = prod(cshape) * steps / wall
(reference src/odil/util.py:408-419), inputs resident in HBM, synthetic (`hat`
reference solution, discrete rhs, zero initial state; poisson.py:21-24,71-86,264-266).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config 4a|5|1|2|3|3b|4b|5b] [--N 512] [--ndim 3]
                  [--dump-outputs DIR] [--full]

A plain run does only what its headline figure needs: set-up, spin-up, the W warm-up steps, the K timed steps,
--dump-outputs if asked, and the JSON line (roofline and kernel_ms from the HIP events of the timed steps themselves).
--full adds everything else the benchmark measures or checks: the CPU baseline before the GPU is touched (unless
--no_cpu_baseline), the per-kernel times of a few extra epochs after the timed ones, the value-level comparison of the
first warm-up epochs with the C oracle's fixture and the multi-GPU loss against the emulated-rank table (`parity_ok`; a
mismatch fails the run), and at the headline size on one GPU the short runs of the other configs (unless
--no_other_configs).  The timed steps themselves are the same with and without it.

--dump-outputs DIR (config 4a on one GPU; bench_outputs/ is git-ignored): after the timed steps, what the timed
optimize_grad call returned after its last step is written as DIR/<name>.npy (dump_outputs below), so that two builds
can be compared output for output.

N > 1: one rank per GPU over RCCL, weak scaling (every rank owns a 512^3 slab of the (N*512, 512, 512) grid;
config 5: a (128, 32, 256, 256) slab of the tracer workload's (128, N*32, 256, 256) grid -- at N = 8 the
256^3 x 128t grid BASELINE.json names, with the domain's own 7 multigrid levels).  Either the caller starts the ranks (`python -m torch.distributed.run
--nproc-per-node N ... bench.py --gpus N`: RANK / WORLD_SIZE are then in the environment), or plain
`python bench.py --gpus N` starts them itself as FRESH child processes before this process has touched the
GPU, relays rank 0's JSON line and exits with the children's status.
Prints ONE JSON line on rank 0.  The other --config values run the remaining BASELINE configs through the
public operator API on one GPU (what bench_configs.py prints, in the driver's JSON contract).
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--config", type=str, default="4a", choices=["4a", "5", "1", "2", "3", "3b", "4b", "4c", "5b"])
    p.add_argument("--N", type=int, default=512)
    p.add_argument("--ndim", type=int, default=3)
    p.add_argument("--dtype", type=str, default="f64", choices=["f64", "f32"])
    p.add_argument("--full", action="store_true",
                   help="also the CPU baseline, the per-kernel epochs, the checks against the references and the other configs")
    p.add_argument("--no_cpu_baseline", action="store_true", help="with --full: skip the CPU baseline")
    p.add_argument("--cpu_N", type=int, default=512, help="grid size of the 1-core CPU-baseline sample (512 = the headline's own: ~5 s "
                   "per epoch of the C port after ~1 min of untimed first-touch page faults of its 8.6 GB)")
    p.add_argument("--cpu_N_all", type=int, default=128, help="grid size per core of the all-cores CPU-baseline leg")
    p.add_argument("--cpu_budget", type=float, default=10.0, help="seconds of timed CPU work per leg")
    p.add_argument("--scale", type=float, default=1.0, help="shrinks the grids of the non-default configs (smoke runs)")
    p.add_argument("--spinup_ms", type=float, default=80.0, help="untimed read-modify-write spin-up before the warm-up steps")
    p.add_argument("--no_other_configs", action="store_true",
                   help="with --full: skip the short runs of the other configs after the timed region")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the timed path returned after its last timed step as DIR/<name>.npy (config 4a, one GPU)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")
    if args.dump_outputs is not None and (args.config != "4a" or args.gpus != 1):
        p.error("--dump-outputs needs --config 4a and --gpus 1")
    return args


def algorithmic_bytes_per_update(ndim, nlvl, wordsize):
    """(10 S + 5) words per fine cell per epoch, S = sum_l 2^(-d l)."""
    S = sum(2.0 ** (-ndim * l) for l in range(nlvl))
    return (10 * S + 5) * wordsize, S


def cpu_baseline(ndim, n_one, n_all, budget_s):
    """The oracle timed on this host, outside the timed region and before this process touches the GPU.
    3-D (the headline): oracle/poisson_epoch.c, the plain-C one-thread restatement of the epoch (pinned to the NumPy
    oracle by tests/test_oracle_c.py), (i) ONE thread -- the reference's default (reference src/odil/runtime.py:8-12) --
    at the headline's own grid, (ii) one worker per host core, concurrently, each on its own grid (what ODIL_MT / one
    process per core can at best deliver); the NumPy oracle (oracle/odil_np.py, the reference's op sequence array by
    array as TF eager runs it) is timed beside it on one thread.  Other ndim: the NumPy oracle only."""
    def leg(cmd, nproc, n, budget):
        start = time.time() + 5.0 + 0.02 * nproc
        cmd = cmd + [str(n), str(budget), str(start)]
        procs = [subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True) for _ in range(nproc)]
        outs = [json.loads(p.communicate()[0].strip().splitlines()[-1]) for p in procs]
        if any(p.returncode for p in procs):
            raise RuntimeError("cpu baseline worker failed")
        return sum(o["cells"] * o["epochs"] / o["seconds"] for o in outs), outs

    numpy_cmd = [sys.executable, "-m", "oracle.cpu_bench", str(ndim)]
    use_c = ndim == 3
    if use_c:
        cmd = [os.path.join(ROOT, "oracle", "_build", "poisson_epoch")]
        try:  # (built by __graft_entry__.build(); rebuilt here when the source is newer or the binary is missing)
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
        except (OSError, subprocess.CalledProcessError) as e:
            if not os.access(cmd[0], os.X_OK):
                print("cpu_baseline: no C port of the epoch ({}); timing the NumPy oracle".format(e), file=sys.stderr)
                use_c = False
    if use_c:
        per_worker, name = 16 * 8.0 * n_all**ndim, "oracle/poisson_epoch.c (plain C, -O3)"
    else:
        cmd, n_one = numpy_cmd, min(n_one, 256 if ndim == 3 else 4096)
        # ~0.35 GB per 128^3 NumPy worker (f64 multigrid state, moments, gradients, temporaries)
        per_worker, name = 0.35e9 * (n_all / 128.0) ** ndim, "oracle/odil_np.py"
    v1, o1 = leg(cmd, 1, n_one, budget_s)
    present = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        import psutil

        avail = psutil.virtual_memory().available
    except Exception:
        avail = 32 << 30
    omp = os.path.join(ROOT, "oracle", "_build", "poisson_epoch_omp")
    if use_c and os.access(omp, os.X_OK) and 16 * 8.0 * n_one**ndim < 0.5 * avail:
        # ONE problem of the headline's own size on all host cores: the same C loops shared among OpenMP threads (pages
        # first touched by the threads that work on them)
        def omp_run(threads, n, budget):
            env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND="spread", OMP_PLACES="threads", OMP_WAIT_POLICY="passive")
            p = subprocess.Popen([omp, str(n), str(budget)], cwd=ROOT, stdout=subprocess.PIPE, text=True, env=env)
            o = json.loads(p.communicate()[0].strip().splitlines()[-1])
            if p.returncode:
                raise RuntimeError("cpu baseline (OpenMP) failed")
            return o

        # how many threads the host really gives this job is not what the affinity mask says (a container's CPU quota is
        # invisible there: 256 threads spinning on a few cores' worth of time ran 3x SLOWER than one): calibrated on a
        # small grid, the thread count with the best rate runs the full-size problem
        cand = sorted({t for t in (4, 8, 16, 32, 64, 128, present) if t <= present})
        rates = {t: (lambda o: o["cells"] * o["epochs"] / o["seconds"])(omp_run(t, min(n_one, 128), 0.4)) for t in cand}
        cores = max(rates, key=rates.get)
        o = omp_run(cores, n_one, budget_s)
        vall = o["cells"] * o["epochs"] / o["seconds"]
        all_sample = ("oracle/poisson_epoch.c with -fopenmp: ONE Poisson {}-D {}^{} f64 multigrid Adam problem on {} threads (best of {} on a "
                      "128^3 calibration; {} cores in the affinity mask), {} epochs in {:.1f} s").format(
                          ndim, n_one, ndim, cores, "/".join(str(t) for t in cand), present, o["epochs"], o["seconds"])
    else:  # one single-thread worker per host core, each on its own (smaller) grid, as many as half of the memory allows
        cores = max(1, min(present, int(0.5 * avail / per_worker)))
        vall, oall = leg(cmd, cores, n_all, budget_s)
        all_sample = "{} concurrent single-thread workers (of {} cores present), each Poisson {}-D {}^{} f64 multigrid Adam, {:.1f} s".format(
            cores, present, ndim, n_all, ndim, max(o["seconds"] for o in oall))
    out = {
        "value": v1,
        "unit": "grid-point-updates/s",
        "cores": 1,
        "kind": "port",
        "sample": "{}, Poisson {}-D {}^{} f64 multigrid Adam, {} epochs in {:.1f} s on one thread".format(
            name, ndim, n_one, ndim, o1[0]["epochs"], o1[0]["seconds"]),
        "all_cores": {"value": vall, "cores": cores, "cores_present": present, "sample": all_sample},
    }
    if use_c:
        vnp, onp_ = leg(numpy_cmd, 1, n_all, min(budget_s, 5.0))
        out["numpy_port"] = {
            "value": vnp, "cores": 1,
            "sample": "oracle/odil_np.py, Poisson {}-D {}^{} f64 multigrid Adam, {} epochs in {:.1f} s on one thread".format(
                ndim, n_all, ndim, onp_[0]["epochs"], onp_[0]["seconds"])}
    return out


def measured_traffic(kernel, ndim, N, dtype):
    """HBM bytes per launch of the dominant kernel from the PMC passes committed under profiles/
    (collected in passes of their own with rocprofv3 --pmc -- FETCH_SIZE / WRITE_SIZE or the TCC_EA0 request counters they
    are derived from -- gfx950 correction applied; the newest round's file first), and the
    file they come from; (None, None) when no profile of this kernel / workload is on record."""
    for name in ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):
        try:
            rec = json.load(open(os.path.join(ROOT, "profiles", name)))
        except OSError:
            continue
        if rec.get("kernel", "").split(" ")[0] == kernel.split(" ")[0] and (ndim, N, dtype) == (3, 512, "f64"):
            return rec["traffic_bytes_per_launch"], "profiles/" + name + " (rocprofv3 --pmc, 512^3 f64 only)"
    return None, None


class _NoEvent:
    def record(self):
        pass


class Timers:
    """HIP-event pairs per kernel family, recorded on the stream the kernels run on.  `only`: the sections that are
    really timed (the others get no events).  Every recorded event is a barrier packet between two launches: with all
    sections of the epoch bracketed, the 512^3 epoch measured 3.21 instead of 2.83 ms (tools/host_enqueue.py), so
    the TIMED region brackets the dominant launch only and the other sections are measured (--full) in a few extra
    epochs after it."""

    def __init__(self, only=None, prealloc=0):
        """prealloc: event pairs created AND recorded once before they are needed.  The runtime grows its pool of
        timing events in chunks; the allocation of the second chunk stalled the queue for 33 ms in the middle of
        whichever launch the ~32nd event of the process bracketed (ODIL_BENCH_DEBUG=1 prints the launch epoch by
        epoch) -- with `--warmup 5 --steps 20` that is a timed epoch, +1.6 ms on the mean of 20."""
        self.pairs, self.only = {}, only
        self.spare = []
        for _ in range(2 * prealloc):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.spare.append(e)
        if prealloc:
            torch.cuda.synchronize()

    def _event(self):
        return self.spare.pop() if self.spare else torch.cuda.Event(enable_timing=True)

    def section(self, name):
        if self.only is not None and name not in self.only:
            return _NoEvent(), _NoEvent()
        a, b = self._event(), self._event()
        self.pairs.setdefault(name, []).append((a, b))
        return a, b

    def summary(self):
        return {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in self.pairs.items()}


def spawn_ranks(ngpus):
    """`python bench.py --gpus N` outside a launcher: start N ranks with torch.distributed.run as a child
    process (this process has not initialised the GPU and never does), pass its output through, return its
    exit status."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ngpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def roofline(kernel, model_bytes, moved_bytes, ms, traffic, traffic_source):
    """`frac` is PHYSICAL: bytes the launch moves (PMC counters when a profile of this exact launch is on record,
    else the bytes it must move) / its HIP-event duration / 8 TB/s.  `frac_model` prices the SURVEY 8(d) minimum-
    traffic model of the work the launch covers -- a fusion credit, it can exceed what any memory system does."""
    phys = traffic if traffic is not None else moved_bytes
    achieved = phys / (ms * 1e-3) / 1e9
    model = model_bytes / (ms * 1e-3) / 1e9
    return {
        "kernel": kernel, "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
        "traffic_source": traffic_source or "none on record for this workload: frac uses compulsory_bytes_per_launch",
        "avg_launch_ms": ms, "algorithmic_bytes_per_launch": model_bytes, "compulsory_bytes_per_launch": moved_bytes,
        "achieved_model": model, "frac_model": model / HBM_PEAK_GBS,
    }


def spin_up(dev, ms):
    """UNTIMED, before the warm-up steps: read-modify-write passes over a 1 GB buffer for `ms` milliseconds.  After
    start-up or ~20 ms of idle the part runs its first epochs 5-15 % slow (2.9, 2.7, 2.6 ... ms for the 512^3 epoch)
    until the memory side has been busy in both directions for a while; fills alone do not end that, read-modify-write
    passes do (tools/idle_ramp2.py).  Not part of any timed region."""
    if ms <= 0:
        return
    buf = torch.zeros(256 << 20, dtype=torch.float32, device=dev)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(8):
            buf.add_(1.0)
        torch.cuda.synchronize()
    del buf


class ApiPoissonRun:
    """The headline workload THROUGH THE PUBLIC API: `examples/poisson/poisson.py` (the reference example's operator
    callback, `Domain` / `Problem`) driven by `odil.util.optimize_grad(args, "adam", problem, state, callback)` --
    reference src/odil/util.py:190-240 -> optimizer.py:286-341.  Same attributes as the bespoke driver
    (`poisson_path.PoissonMultigridAdam`, timed here up to round 5; tools/headline_ab.py holds the two side by side)."""

    def __init__(self, ndim, N, dtype, dev, ref_u=None):
        sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
        import odil_amd as odil
        import poisson
        from odil_amd import ops

        self.odil = odil
        odil.util.set_log_file(open(os.devnull, "w"))
        self.args = poisson.parse_args(["--ndim", str(ndim), "--N", str(N), "--double", "1" if dtype == torch.float64 else "0"])
        self.problem, self.state = poisson.make_problem(self.args)
        if ref_u is not None:
            # the fixture's inputs bit for bit: the example forms its reference solution on the device (torch pow: last-bit
            # differences from NumPy's, which this problem amplifies to O(1) within three epochs)
            h2 = [np.float64(1.0 / N) ** 2] * ndim
            rhs, _ = ops.poisson_residual(ref_u, torch.zeros_like(ref_u), h2)
            assert not self.problem._fused_checked
            self.problem.extra.rhs = rhs
        self.ref_u = ref_u if ref_u is not None else self.problem.extra.ref_u
        self.problem.eval_loss_grad_device(self.state)  # (the operator is recognised here: fused HIP route)
        self.ev = self.problem._fused
        assert self.ev is not None, "the Poisson operator must take the fused HIP route"
        self.nlvl = self.ev.nlvl
        self.local_cells = self.global_cells = int(np.prod(self.problem.domain.cshape))
        self.n_unknowns_local = sum(self.ev.sizes)
        self.w = self.problem.domain.arrays_from_state(self.state)
        self.mw = self.vw = None
        self.done = 0
        self._loss = None

    def _call(self, epochs, callback):
        a = self.args
        a.epoch_start, a.epochs = 0, epochs
        moments = None if self.mw is None else (self.mw, self.vw)
        arrays, info = self.odil.util.optimize_grad(a, "adam", self.problem, self.state, callback, moments=moments,
                                                    steps_done=self.done)
        self.w, self.mw, self.vw = arrays, [t.clone() for t in info.m], [t.clone() for t in info.v]
        self.done += epochs

    def epoch(self, timers=None):
        """One epoch as a call of its own (warm-up: every call also makes the driver's initial evaluation)."""
        self.ev.timers = timers
        seen = []
        self._call(1, lambda st, ep, pinfo: seen.append(pinfo))
        self.ev.timers = None
        self._loss = seen[-1]["loss"]

    def timed(self, steps, timers, barrier):
        """EXACTLY `steps` optimizer steps of ONE `optimize_grad` call between two barriers (the driver's per-epoch callback
        brackets them: the call's own set-up -- packed copy, moments, the initial evaluation for the callback -- lies
        before the first barrier); -> seconds."""
        marks, seen = [], []

        def cb(st, ep, pinfo):
            seen.append(pinfo)
            if ep == 0:
                self.ev.timers = timers
                barrier()
                marks.append(time.perf_counter())
            elif ep == steps:
                barrier()
                marks.append(time.perf_counter())
                self.ev.timers = None

        self._call(steps, cb)
        self._loss = seen[-1]["loss"]
        return marks[1] - marks[0]

    def last_loss(self):
        return float(np.array(self._loss))


DUMP_SAMPLE = 1 << 18  # entries stored of a larger multigrid level (a seeded sample)
DUMP_LIMIT = 64 << 20  # bytes of all dumped arrays together


def dump_outputs(path, run):
    """--dump-outputs: what the timed `optimize_grad` call returned after its last step -- the unknowns of every multigrid
    level (`x_l<k>`) and Adam's two moments (`m_l<k>`, `v_l<k>`) in the run's dtype -- and the loss the driver's callback
    received for that step (`loss`, float64), as `path`/<name>.npy.  A level of more than DUMP_SAMPLE entries is stored
    as a fixed sample: sorted flat indices drawn with seed k (the same positions in every run of that shape), stored
    beside it as `sample_index_l<k>` (float64, exact).  The inputs of the run are the same from run to run (zero start,
    the example's deterministic reference solution), so two builds can be compared file by file.  -> {name: shape}."""
    files = {"loss": np.array([run.last_loss()], dtype=np.float64)}
    for lvl, (x, m, v) in enumerate(zip(run.w, run.mw, run.vw)):
        take = lambda t: t.reshape(-1)
        if x.numel() > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(lvl).choice(x.numel(), DUMP_SAMPLE, replace=False))
            files["sample_index_l{}".format(lvl)] = idx.astype(np.float64)
            ti = torch.as_tensor(idx, device=x.device)
            take = lambda t, ti=ti: t.reshape(-1)[ti]
        for name, t in (("x", x), ("m", m), ("v", v)):
            files["{}_l{}".format(name, lvl)] = take(t.detach()).cpu().numpy()
    total = sum(a.nbytes for a in files.values())
    assert total <= DUMP_LIMIT, "--dump-outputs: {} bytes exceed the {} byte limit".format(total, DUMP_LIMIT)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    os.makedirs(path, exist_ok=True)
    for name, a in files.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {name: list(a.shape) for name, a in files.items()}


def run_poisson(args, rank, world, dev, comm, barrier):
    from odil_amd.slab import SlabPoissonAdam

    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    ndim, N = args.ndim, args.N
    if world > 1:
        # weak scaling: every rank owns an N^3 slab of the (world*N, N, N) grid
        assert ndim == 3, "the slab decomposition is 3-D"
        run = SlabPoissonAdam(N, rank, world, dtype=dtype, device=dev)
        step = lambda timers=None: run.epoch(comm, timers)
    else:
        ref_u = None
        if (ndim, N, args.dtype) == (3, 512, "f64"):
            # the headline at N = 1 starts from the inputs of the value-level fixture, bit for bit (reference solution by
            # NumPy on the host, right-hand side from it by the residual kernel): its first epochs are then comparable
            # with the C oracle's (oracle_values_check) -- a last-bit change of the inputs is amplified to O(1) within
            # three epochs of this problem
            ref_u = torch.as_tensor(hat_reference_host(N)).to(dev)
        run = ApiPoissonRun(ndim, N, dtype, dev, ref_u=ref_u)
        del ref_u
        step = lambda timers=None: run.epoch(timers)
    # (created and primed before the warm-up: growing the runtime's event pool stalls the queue, see Timers)
    timers = Timers(only=("adjoint_transpose", "adjoint", "adam"), prealloc=2 * args.steps + 8)
    import gc

    gc.collect()
    gc.disable()  # (a collection of the interpreter in the middle of the loop starves the queue: see DESIGN section 5)
    spin_up(dev, args.spinup_ms)
    oracle = None
    for k in range(args.warmup):
        step()
        if args.full and world == 1:  # the run starts from the zero state: its first epochs ARE the epochs of the value-level fixture
            oracle = oracle_values_check(run, k + 1, oracle, (ndim, N, args.dtype))
    dumped = None
    if world == 1:
        elapsed = run.timed(args.steps, timers, barrier)
        if args.dump_outputs is not None:  # (after the timed region, before any further epoch)
            dumped = dump_outputs(args.dump_outputs, run)
    else:
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(timers)
        barrier()
        elapsed = time.perf_counter() - t0
    gc.enable()
    loss = run.last_loss(comm) if world > 1 else run.last_loss()
    kt = dict()
    if args.full:
        every = Timers(prealloc=8 * 5)  # the other sections: a few epochs outside the timed region (events primed: see Timers)
        if world == 1:
            run.timed(5, every, barrier)
        else:
            for _ in range(5):
                step(every)
        barrier()
        kt = every.summary()
    wordsize = 8 if dtype == torch.float64 else 4
    kt.update(timers.summary())
    if os.environ.get("ODIL_BENCH_DEBUG") and rank == 0:  # the dominant launch epoch by epoch (clock ramp, outliers)
        for name, pairs in timers.pairs.items():
            print(name, " ".join("%.2f" % a.elapsed_time(b) for a, b in pairs), file=sys.stderr)
    tname = "double" if wordsize == 8 else "float"
    if "adjoint_transpose" in kt:
        # Dominant kernel: stencil adjoint + first transposed prolongation + the Adam updates of levels 0 and
        # 1 in one launch.  Model bytes of the work this launch covers: stencil adjoint 2 words
        # (read r, write g) + first level of the P^T chain 1 + 1/8 (read g, write g1) + Adam 7 words per unknown
        # of levels 0 and 1 (7 + 7/8) = 11 words per fine cell.  The launch itself moves less -- g never reaches
        # memory: read fu; read + write x, m, v of level 0; write g1 and read + write x, m, v of level 1 =
        # 7 + 7/8 words.
        # (rocprofv3 lists it with its template arguments: <T, 1/h^2 as a product, g0 not stored>)
        kernel = "k_poisson_adjoint_tile<{}, true, false> (adjoint + first P^T + Adam of levels 0 and 1)".format(tname)
        model = 11.0 * run.local_cells * wordsize
        moved = (7.0 + 7.0 / 8.0) * run.local_cells * wordsize
        ms = kt["adjoint_transpose"]
    elif kt.get("adjoint", 0) > kt.get("adam", 0):
        # adjoint with the finest-level Adam update fused in: read fu, x, m, v; write gu, x, m, v
        kernel = "k_poisson_adjoint<{}, true> (+Adam of the finest level)".format(tname)
        model = moved = 8.0 * run.local_cells * wordsize
        ms = kt["adjoint"]
    else:
        kernel = "k_adam<{}>".format(tname)
        model = moved = 7.0 * run.n_unknowns_local * wordsize
        ms = kt["adam"]
    traffic, source = measured_traffic(kernel, ndim, N, args.dtype) if world == 1 else (None, None)
    abytes, S = algorithmic_bytes_per_update(ndim, run.nlvl, wordsize)
    return dict(
        elapsed=elapsed, cells=run.global_cells, loss=loss, kernel_ms=kt,
        metric="grid-point-updates/s, Poisson {}^{} multigrid".format(N, ndim),
        workload=("3D Poisson 512^3 multigrid (9 levels) Adam epoch, {}".format(
            "1xMI355X, public operator API (odil.util.optimize_grad on examples/poisson/poisson.py)" if world == 1
            else "512^3 slab per GPU x {} MI355X".format(world))
            if (ndim, N) == (3, 512) else "{}D Poisson {}^{} multigrid Adam epoch".format(ndim, N, ndim)),
        config=dict(cells_per_gpu=run.local_cells, levels=run.nlvl, optimizer="adam lr=0.005"),
        roofline=roofline(kernel, model, moved, ms, traffic, source), abytes=abytes, dtype=args.dtype,
        exchanges_per_epoch=2 if world > 1 else 0, oracle=oracle, dumped=dumped)


def hat_reference_host(N):
    """The reference solution 'hat' (reference examples/poisson/poisson.py:18-24) on the cell centres of the unit cube,
    float64, NumPy on the host -- the SAME arithmetic as tests/golden/make_golden_fullsize.py:reference_u (same image,
    same libm: same bits), so that this run's inputs are the fixture's."""
    import numpy as np

    x = (np.arange(N, dtype=np.float64) + 0.5) / N
    p = (1 - x) * x * 5
    u = np.ones((N, N, N))
    u *= p[:, None, None]
    u *= p[None, :, None]
    u *= p[None, None, :]
    u5 = u**5
    return (u5 / (1 + u5)) ** (1 / 5)


def oracle_values_check(run, epoch, acc, key):
    """--full: VALUE-level parity inside the bench run (N = 1, headline size only): the losses of the first epochs (untimed warm-up;
    zero start) and 64 sampled unknowns per level after the last recorded epoch against tests/golden/fullsize_poisson_N512.npz
    -- three epochs of the plain-C oracle at 512^3 (tests/golden/make_golden_fullsize.py; the oracle itself is NOT run
    here).  Inputs are the fixture's bit for bit (checked on its sampled entries).  Tolerances: loss 1e-10; unknowns 1e-6
    of a level's largest sample (tests/test_fullsize_values_gpu.py explains what the problem's conditioning leaves of
    two correct float64 implementations after epoch 1: observed 7e-10).  Returns the accumulated record (None when no
    fixture applies)."""
    if key != (3, 512, "f64"):
        return None
    path = os.path.join(ROOT, "tests", "golden", "fullsize_poisson_N512.npz")
    if acc is None:
        if epoch != 1 or not os.path.exists(path):
            return None
        import numpy as np

        fx = np.load(path)
        acc = {"source": "tests/golden/fullsize_poisson_N512.npz (oracle/poisson_epoch.c, 3 epochs at 512^3)", "tol": 1e-10,
               "loss_rel_err": [], "ok": True, "_fx": {k: fx[k] for k in fx.files}}
        i0 = torch.as_tensor(fx["sample_index"][: int(fx["sample_count"][0])], device=run.ref_u.device)
        acc["inputs_bit_identical"] = bool(
            np.array_equal(run.ref_u.reshape(-1)[i0].cpu().numpy(), fx["ref_u_samples"])
            and np.array_equal(run.ev.rhs.reshape(-1)[i0].cpu().numpy(), fx["rhs_samples"]))
        if not acc["inputs_bit_identical"]:
            # another math library than the fixture's host (a last-bit difference of ref_u): on this problem that alone moves
            # the third epoch by percent -- the comparison would measure the inputs, not the kernels.  Reported, not judged.
            acc.update(ok=None, note="inputs differ from the fixture's in the last bits (another libm?): comparison skipped")
            acc.pop("_fx")
            return acc
    fx = acc.get("_fx")
    if fx is None or epoch > int(fx["epochs"]):
        return acc
    import numpy as np

    want, got = float(fx["losses"][epoch - 1]), run.last_loss()
    err = abs(got - want) / abs(want)
    acc["loss_rel_err"].append(err)
    acc["ok"] = bool(acc["ok"] and err <= acc["tol"])
    if epoch == int(fx["epochs"]):
        idx = np.split(fx["sample_index"], np.cumsum(fx["sample_count"])[:-1])
        ref = np.split(fx["x_samples_e{}".format(epoch)], np.cumsum(fx["sample_count"])[:-1])
        by_level = []
        for w, i, r in zip(run.w, idx, ref):
            g = w.reshape(-1)[torch.as_tensor(i, device=w.device)].cpu().numpy()
            by_level.append(float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-300)))
        worst = max(by_level)
        acc["x_sample_rel_err_after_epoch_{}".format(epoch)] = worst
        acc["x_sample_rel_err_by_level"] = by_level
        acc["ok"] = bool(acc["ok"] and worst <= 1e-6)
        acc["epochs"] = epoch
        del acc["_fx"]
    return acc


def make_tracer_rank(args, rank, world, dev):
    """One rank of BASELINE config 5 (velocity from tracer with three space dimensions, slab-decomposed along x):
    (SlabTracedAdam, (nt, nx_rank, ny), levels, parsed example arguments)."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "velocity_from_tracer"))
    import odil_amd as odil
    import veltracer3d
    from odil_amd.slab_traced import SlabTracedAdam, shape_state

    sc = lambda n: max(8, int(round(n * args.scale)) // 8 * 8)
    nt, nx_rank, ny = sc(128), sc(32), sc(256)
    odil.util.set_log_file(open(os.devnull, "w"))
    # the domain's own level count (min over the axes of log2 n, reference core.py:66-73): levels that leave a rank
    # fewer than 2 cells of x are agglomerated by slab_traced.py
    a = veltracer3d.parse_args(["--Nt", str(nt), "--Nx", str(nx_rank * world), "--Ny", str(ny), "--Nz", str(ny)])
    dtype = np.float32
    domain = odil.Domain(cshape=(a.Nt, a.Nx, a.Ny, a.Nz), dimnames=("t", "x", "y", "z"), lower=(0, 0, 0, 0),
                         upper=(1, 1, 1, 1), dtype=dtype, multigrid=a.multigrid, mg_interp=a.mg_interp, mg_nlvl=a.nlvl)
    x, y, z = np.meshgrid(*domain.points_1d("x", "y", "z"), indexing="ij")
    extra = argparse.Namespace(args=a)
    extra.u_init = domain.mod.cast(veltracer3d.blob(x, y, z, 0), dtype)
    extra.u_final = domain.mod.cast(veltracer3d.blob(x, y, z, 1), dtype)
    del x, y, z
    state = odil.State()
    for key in ("u",) + veltracer3d.VEL:
        state.fields[key] = odil.Field(None, loc=veltracer3d.LOC)
    problem = odil.Problem(veltracer3d.operator, domain, extra)
    nlvl = domain.mg_nlvl
    run = SlabTracedAdam(problem, shape_state(domain, state), rank, world, lr=a.lr, device=dev)
    return run, (nt, nx_rank, ny), nlvl, a


def run_tracer(args, rank, world, dev, comm, barrier):
    """BASELINE config 5: velocity from tracer with three space dimensions, slab-decomposed along x."""
    run, (nt, nx_rank, ny), nlvl, a = make_tracer_rank(args, rank, world, dev)
    timers = Timers(only=("forward",), prealloc=args.steps + 4)
    import gc

    gc.collect()
    gc.disable()  # (as in run_poisson)
    spin_up(dev, args.spinup_ms)
    for _ in range(args.warmup):
        run.epoch(comm)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run.epoch(comm, timers)
    barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    loss = run.last_loss(comm)
    kt = dict()
    if args.full:  # the other sections: two epochs outside the timed region
        every = Timers(prealloc=8 * 2)
        for _ in range(2):
            run.epoch(comm, every)
        barrier()
        kt = every.summary()
    kt.update(timers.summary())
    nsrc, ncot = len(run.kern.src_keys), len(run.kern.cot)
    moved = float(nsrc + ncot) * run.local_cells * 4  # reads each field once (neighbours are cache hits), writes the cotangents
    return dict(
        elapsed=elapsed, cells=run.global_cells, loss=loss, kernel_ms=kt,
        metric="grid-point-updates/s, velocity_from_tracer {}^3 x {}t".format(ny, nt),
        workload="3D velocity_from_tracer (t,x,y,z) = ({},{},{},{}) slab per GPU x {} MI355X, Adam epoch, f32, {} levels".format(
            nt, nx_rank, ny, ny, world, nlvl),
        config=dict(cells_per_gpu=run.local_cells, levels=nlvl, optimizer="adam lr={}".format(a.lr), fields=4),
        roofline=roofline("k_fwd (generated: residuals + reverse pass, {} fields in, {} cotangent arrays out)".format(nsrc, ncot),
                          moved, moved, kt["forward"], None, None),
        abytes=None, dtype="f32", exchanges_per_epoch=4 if world > 1 else 0)


def pmc_traffic(path):
    """{kernel: HBM bytes per launch} of the generated kernels from a committed rocprofv3 summary (tools/prof_cfg.sh with
    HBM=1: TCC_EA0_RDREQ[_32B] / WRREQ[_64B] summed over the channels.  MI355X_MICROARCH.md, HBM section: on gfx950 a
    read request of a coalesced stream is a 128-byte request tallied at 64 B -- FETCH_SIZE must be doubled -- so reads are
    priced at 128 B per non-32-byte request; writes at 64 / 32 B per request, which the guide calls uncalibrated: they
    reproduce the bytes these kernels store to within 15 %), or None when the file is not on record."""
    import re

    try:
        text = open(path).read()
    except OSError:
        return None
    res = dict()
    for line in text.splitlines():
        if "TCC_EA0_RDREQ_sum" not in line:
            continue
        name = line.split()[0]
        val = lambda c: float(re.search(c + r": max ([0-9.e+]+)", line).group(1))
        rd, rd32, wr, wr64 = val("TCC_EA0_RDREQ_sum"), val("TCC_EA0_RDREQ_32B_sum"), val("TCC_EA0_WRREQ_sum"), val("TCC_EA0_WRREQ_64B_sum")
        res[name] = {"read_bytes": (rd - rd32) * 128 + rd32 * 32, "write_bytes": wr64 * 64 + (wr - wr64) * 32, "source": os.path.basename(path)}
    return res or None


def other_configs(args, dev):
    """--full, after the timed region of the default run (N = 1 only, outside every timed window): a few epochs each of the
    other single-GPU BASELINE workloads, so that the driver's record carries them -- 3b heat inverse 256 x 512^2
    (traced operator, Adam), 5 the tracer workload's per-rank slab (128, 32, 256, 256) as one rank, 4b one Newton step
    of Poisson 512^3 with the geometric-multigrid solve.  ms_per_step by HIP events around the steps after a warm-up
    step; frac_model prices the SURVEY 8(d) minimum-traffic model of an Adam epoch against 8 TB/s."""
    import copy
    import gc

    out = dict()

    def timed(step, nwarm, nsteps):
        for _ in range(nwarm):
            step()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(nsteps):
            step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / nsteps

    def attempt(name, fn):
        t0 = time.perf_counter()
        try:
            out[name] = fn()
        except Exception as e:  # the headline line must not depend on these
            out[name] = {"error": "{}: {}".format(type(e).__name__, str(e).splitlines()[0] if str(e) else "")}
        out[name]["wall_s"] = time.perf_counter() - t0
        gc.collect()
        torch.cuda.empty_cache()

    def heat():
        import bench_configs
        import odil_amd as odil

        modname, argv, optname, _, _, name = bench_configs.CONFIGS["3b"]
        sc = lambda n: max(8, int(round(n * args.scale)) // 8 * 8)
        import importlib

        ex = importlib.import_module(modname)
        a = ex.parse_args(argv(sc))
        odil.util.set_log_file(open(os.devnull, "w"))
        problem, state = ex.make_problem(a)
        loss_grad = odil.util.make_loss_grad(problem, state)
        opt = odil.optimizer.AdamNativeOptimizer(dtype=problem.domain.dtype, mod=problem.domain.mod)
        arrays = problem.domain.arrays_from_state(state)
        carry = dict(x=arrays, m=None, done=0)

        per_call = 10  # epochs per optimizer call (a call's own set-up is ~0.4 ms here: 3.7 ms per epoch of 1-epoch calls)

        def step():
            x, info = opt.run(carry["x"], loss_grad, epochs=per_call, lr=a.lr, moments=carry["m"], steps_done=carry["done"])
            carry.update(x=x, m=(info.m, info.v), done=carry["done"] + per_call)

        ms = timed(step, 1, 2) / per_call
        cells = int(np.prod(problem.domain.cshape))
        nout = len(problem.eval_loss_grad(state)[2])
        model = bench_configs.model_bytes_per_update(problem, state, "adam", nout)
        return {"workload": name.format(problem.domain.cshape[0], problem.domain.cshape[-1]), "ms_per_step": ms,
                "value": cells / (ms * 1e-3), "frac_model": cells * model / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "traced": problem._traced is not None}

    def tracer():
        from odil_amd.slab import LocalComm

        sub = copy.copy(args)
        sub.steps, sub.warmup, sub.spinup_ms = 5, 2, 0.0
        res = run_tracer(sub, 0, 1, dev, LocalComm(), torch.cuda.synchronize)
        ms = 1e3 * res["elapsed"] / sub.steps
        # SURVEY 8(d) model of an Adam epoch with k = 4 multigrid fields and 8 outputs, S = 16 / 15
        S = sum(2.0 ** (-4 * l) for l in range(res["config"]["levels"]))
        model = (4 * (10 * S + 2) + 2 * 8 + 1) * 4
        return {"workload": res["workload"], "ms_per_step": ms, "value": res["cells"] / (ms * 1e-3),
                "frac_model": res["cells"] * model / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "kernel_ms": res["kernel_ms"],
                "traced": True}  # (SlabTracedAdam runs generated kernels only: it has no autograd path)

    def newton(modname="poisson", argv=None, env=None, name=None, words_per_cycle=(4 * 3 + 2.125), words_setup=0.0,
               words_moved=None):
        """One Newton step (the SECOND of two: work buffers exist) of a 3-D problem through `odil.util.optimize`.
        env: switches for the step (ODIL_NEWTON_SHORTCUT=0: the general route eval_operator_grad -> linearize ->
        linsolver.solve instead of the recognised-Poisson shortcut; ODIL_GMG=stencil: the variable-coefficient cycle)."""
        def run():
            import importlib

            import bench_configs
            import odil_amd as odil

            sc = lambda n: max(8, int(round(n * args.scale)) // 8 * 8)
            av = argv(sc) if argv is not None else bench_configs.CONFIGS["4b"][1](sc)
            saved = {k: os.environ.get(k) for k in (env or {})}
            os.environ.update(env or {})
            try:
                ex = importlib.import_module(modname)
                a = ex.parse_args(av)
                odil.util.set_log_file(open(os.devnull, "w"))
                problem, state = ex.make_problem(a)
                a.epoch_start, a.epochs = 0, 1

                def step():
                    # every timed step is the FIRST Newton step from the zero state (a step from the converged state
                    # would iterate on rounding noise until it stagnates: twice the cycles, not the workload)
                    for f in state.fields.values():
                        f.array.zero_()
                    odil.util.optimize(a, "newton", problem, state, None)

                ms = timed(step, 2, 2)  # (two warm steps: the solver kept with the domain allocates its own coefficient buffer in the second)
                cells = int(np.prod(problem.domain.cshape))
                # bytes model of one Newton step with a geometric-multigrid solve (words per fine cell): per V-cycle four
                # smoothing sweeps + the residual with its restriction, over all levels (x 8/7) -- 3 and 2 1/8 words for
                # the constant-coefficient Poisson cycle, 10 and 9 1/8 with seven coefficient arrays --; per step the
                # residual (3), the update x += delta (3), the first iterate by nested iteration (one cycle's worth) and
                # `words_setup` (general route: the seven coefficient arrays written by eval_operator_grad, read by
                # linearize / recognition, the coarse operators formed); the cycle count comes from the solver's own
                # status of one more (untimed) step
                seen = []
                a.epochs = 1
                for f in state.fields.values():
                    f.array.zero_()
                odil.util.optimize(a, "newton", problem, state, lambda s, e, p: seen.append(p.get("linsolver")))
                st = next((st for st in seen if st and "niter" in st), None)
                cycles = None if st is None else int(st["niter"])
                wsize = 8.0 if np.dtype(problem.domain.dtype) == np.float64 else 4.0
                model = None if cycles is None else (words_per_cycle * 8.0 / 7.0 * (cycles + 1) + 6 + words_setup) * wsize
                return {"workload": (name or bench_configs.CONFIGS["4b"][5]).format(problem.domain.cshape[0], problem.domain.cshape[-1]),
                        "ms_per_step": ms, "value": cells / (ms * 1e-3), "vcycles": cycles,
                        "solver": None if st is None else st.get("method"), "model_bytes_per_update": model,
                        # (what the cycle's launches really stream per fine cell: sweeps in pairs, one pass per pair)
                        "words_moved_per_cycle": words_moved,
                        "frac_model": None if model is None else cells * model / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "loss_after": float(problem.eval_loss_grad(state)[0]), "env": env or {},
                        "vram_peak_gb": torch.cuda.max_memory_allocated() / 1e9}
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return run

    def api(key, epochs, warmup):
        """Configs 1, 2, 5b through the public operator API (bench_configs.run_config), a few epochs each."""
        def run():
            import bench_configs

            out = bench_configs.run_config(key, args.scale, epochs=epochs, warmup=warmup)
            model = out.get("model_bytes_per_update")
            ms = out["ms_per_epoch"]
            whole = {k: out[k] for k in ("us_per_epoch_whole_epochs_in_one_launch", "whole_epochs_kernel") if k in out}
            timing = "median of {} epochs, HIP events in the driver's per-epoch callback".format(out["epochs"])
            if "us_per_epoch_whole_epochs_in_one_launch" in whole:
                # a problem of one workgroup: the driver's per-epoch callback forces one launch PER epoch; a run as the
                # examples make it (no callback, or util.make_callback, which tells its cadence) is what a step costs
                whole["ms_per_step_with_a_per_epoch_callback"] = ms
                ms = 1e-3 * whole["us_per_epoch_whole_epochs_in_one_launch"]
                timing = ("wall clock of one optimize() call of 4000 epochs without a per-epoch callback / 4000 (whole epochs "
                          "in one launch, the call's set-up included); " + timing + ": ms_per_step_with_a_per_epoch_callback")
            return {"workload": out["name"], "ms_per_step": ms, "value": out["cells"] / (ms * 1e-3), "optimizer": out["optimizer"],
                    **whole, "model_bytes_per_update": model,
                    "frac_model": None if not model else out["cells"] * model / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "loss_after": out["loss"], "timing": timing,
                    "ms_mean": out["ms_mean"], "ms_max": out["ms_max"], "ms_min": out["ms_min"], "setup_s": out["setup_s"],
                    "traced": out["traced"], "fused": out["fused"], "vram_peak_gb": out["vram_peak_gb"],
                    "vram_reserved_gb": out["vram_reserved_gb"]}
        return run

    for sub in ("poisson", "heat", "velocity_from_tracer"):
        sys.path.insert(0, os.path.join(ROOT, "examples", sub))
    for sub in ("diffusion",):
        sys.path.insert(0, os.path.join(ROOT, "examples", sub))
    # (the Newton configurations first: after the 65 GB of the tracer configurations the same steps measure ~8 % slower --
    # 43 against 39.5 ms for 4b on one box, tools/oc_ab.py -- in whatever physical pages the allocator is handed then)
    attempt("4b", newton(words_moved=3 + 2.125 + 2.125 + 3))  # pre pair, restricted residual, x + P x_c, post pair
    # the same Newton step WITHOUT the recognised-Poisson shortcut: eval_operator_grad (seven coefficient arrays) ->
    # linearize_device -> linsolver.solve -> recognise -> V-cycles; then with the constant-coefficient cycle switched off
    # as well (the cycle any (2 d + 1)-point operator gets), and that cycle on a genuinely variable operator at 256^3
    attempt("4b_general", newton(env={"ODIL_NEWTON_SHORTCUT": "0"}, name="poisson 3D {0}^3 newton, general route (linearize + solve) f64",
                                 words_setup=7 * 3, words_moved=3 + 2.125 + 2.125 + 3))
    attempt("4b_varcoef", newton(env={"ODIL_NEWTON_SHORTCUT": "0", "ODIL_GMG": "stencil"}, words_per_cycle=4 * 10 + 9.125,
                                 words_setup=7 * 3 + 8, words_moved=2 * 10 + 9.125 + 2.125,
                                 name="poisson 3D {0}^3 newton, variable-coefficient multigrid f64"))
    attempt("4c_diffusion", newton("diffusion", lambda sc: ["--ndim", "3", "--N", str(sc(256)), "--kind", "jump", "--linsolver",
                                                             "multigrid", "--linsolver_tol", "1e-10"],
                                   words_per_cycle=4 * 10 + 9.125, words_setup=7 * 3 + 8, words_moved=2 * 10 + 9.125 + 2.125,
                                   name="diffusion div(k grad u), k jumps 1 : 1000, 3D {0}^3 newton + variable-coefficient multigrid f64"))
    # the same solves with float32 V-cycles inside a float64 residual loop (gmg.solve_mixed; ODIL_GMG_MIXED=1: opt-in -- the
    # entries above are float64 throughout): same tolerance on the float64 residual, the cycles' traffic halved
    attempt("4b_mixed", newton(env={"ODIL_GMG_MIXED": "1"}, words_per_cycle=(4 * 3 + 2.125) / 2 + 3 + 2.5,
                               name="poisson 3D {0}^3 newton + gmg, float32 cycles / float64 residual"))
    attempt("4b_varcoef_mixed", newton(env={"ODIL_NEWTON_SHORTCUT": "0", "ODIL_GMG": "stencil", "ODIL_GMG_MIXED": "1"},
                                       words_per_cycle=(4 * 10 + 9.125) / 2 + 10 + 2.5, words_setup=7 * 3 + 8 + 7 * 1.5,
                                       name="poisson 3D {0}^3 newton, variable-coefficient multigrid, float32 cycles / float64 residual"))
    attempt("4c_diffusion_mixed", newton("diffusion", lambda sc: ["--ndim", "3", "--N", str(sc(256)), "--kind", "jump", "--linsolver",
                                                                   "multigrid", "--linsolver_tol", "1e-10"], env={"ODIL_GMG_MIXED": "1"},
                                         words_per_cycle=(4 * 10 + 9.125) / 2 + 10 + 2.5, words_setup=7 * 3 + 8 + 7 * 1.5,
                                         name="diffusion 3D {0}^3 newton, variable-coefficient multigrid, float32 cycles / float64 residual"))
    attempt("3b", heat)
    attempt("5_one_rank", tracer)
    attempt("4a_api", api("4a", 20, 3))  # the headline workload through odil.util.optimize(args, "adam", problem, state, cb)
    attempt("1", api("1", 400, 2))
    attempt("2", api("2", 30, 1))
    attempt("5b", api("5b", 10, 2))
    # HBM traffic of the dominant generated launches from the counter passes on record (profiles/, same commands)
    for key, fname in (("3b", "r05_heat2d_pmc.txt"), ("5_one_rank", "r05_cfg5_pmc.txt")):
        if key in out and "error" not in out[key]:
            out[key]["traffic"] = pmc_traffic(os.path.join(ROOT, "profiles", fname))
    return out


def run_api(args, dev):
    """Configs 1, 2, 3, 3b, 4b, 5b through the public operator API (bench_configs.py) on one GPU."""
    import bench_configs

    spin_up(dev, args.spinup_ms)
    out = bench_configs.run_config(args.config, args.scale, epochs=args.steps, warmup=args.warmup)
    model = out.get("model_bytes_per_update")
    ms = out["ms_per_epoch"]
    rl = None
    if model:
        rl = roofline("whole epoch (all launches; SURVEY 8(d) model bytes -- no single dominant launch timed)",
                      model * out["cells"], model * out["cells"], ms, None, None)
    return dict(elapsed=1e-3 * out["ms_mean"] * out["epochs"], cells=out["cells"], loss=out["loss"], kernel_ms={},
                metric="grid-point-updates/s, " + out["name"], workload=out["name"] + ", 1xMI355X, public operator API",
                config=dict(cells_per_gpu=out["cells"], optimizer=out["optimizer"],
                            **{k: out[k] for k in ("us_per_epoch_whole_epochs_in_one_launch",) if k in out}), roofline=rl,
                abytes=model,
                dtype=out["dtype"], exchanges_per_epoch=0, steps=out["epochs"])


def check_parity(args, res, world):
    """--full: the run checks ITSELF: the (all-reduced) loss after warmup + steps epochs against profiles/expected_losses.json --
    the same deterministic workload with its ranks emulated on one GPU (tools/expected_losses.py: device copies instead
    of RCCL messages, the same kernels).  A wrong halo, a reused receive buffer or a missed wait on the first real
    multi-GPU run changes the trajectory and fails here instead of printing a plausible number.  None: no reference for
    this configuration (other sizes / more epochs than recorded)."""
    key = {"4a": "poisson_512", "5": "tracer_cfg5"}.get(args.config)
    if key is None or args.scale != 1.0 or (args.config == "4a" and (args.ndim, args.N, args.dtype) != (3, 512, "f64")):
        return None
    if args.config == "4a" and world == 1:
        return None  # N = 1 is held to the C oracle's VALUES instead (oracle_values_check); the table is these kernels' own
    try:
        table = json.load(open(os.path.join(ROOT, "profiles", "expected_losses.json")))
    except OSError:
        return None
    ref, k = table.get(key, dict()).get(str(world)), args.warmup + args.steps
    if not ref or not 1 <= k <= len(ref):
        return None
    want, got = float(ref[k - 1]), float(res["loss"])
    tol = 1e-9 if res["dtype"] == "f64" else 1e-4  # (the trajectory is bit-identical by construction: only the order of the
    err = abs(got - want) / abs(want)             # ranks' partial sums in the all-reduce of the LOSS differs)
    return {"ok": bool(err <= tol), "rel_err": err, "expected": want, "tol": tol, "epoch": k,
            "source": "profiles/expected_losses.json ({} ranks emulated on one GPU)".format(world)}


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    cpu = None
    if args.full and not args.no_cpu_baseline and world == 1:  # child processes: started before this process initialises the GPU
        cpu = cpu_baseline(args.ndim if args.config == "4a" else 3, args.cpu_N, args.cpu_N_all, args.cpu_budget)
    from odil_amd.slab import LocalComm

    comm = LocalComm()
    dist = None
    if world > 1:
        import torch.distributed as dist

        from odil_amd.slab import TorchDistComm

        backend = os.environ.get("ODIL_DIST_BACKEND", "nccl")  # nccl == RCCL on ROCm
        ngpu = torch.cuda.device_count()
        local_rank = local_rank % max(ngpu, 1)  # (tests may oversubscribe one GPU with gloo)
        torch.cuda.set_device(local_rank)
        # No silent fallback: a rank that cannot initialise RCCL fails the job (gloo, which stages the planes
        # through the host, only when ODIL_DIST_BACKEND asks for it -- the CPU-side tests do).
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
        assert dist.get_world_size() == world
        if args.gpus != world:
            raise SystemExit("bench.py: --gpus {} but WORLD_SIZE={}".format(args.gpus, world))
        comm = TorchDistComm(rank, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU (the product has no CPU path)"
    dev = torch.device("cuda", local_rank)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    others = None
    if args.config == "4a":
        res = run_poisson(args, rank, world, dev, comm, barrier)
        if args.full and world == 1 and not args.no_other_configs and (args.ndim, args.N) == (3, 512):
            res_run = res.pop("run", None)
            del res_run
            torch.cuda.empty_cache()
            others = other_configs(args, dev)
    elif args.config == "5":
        res = run_tracer(args, rank, world, dev, comm, barrier)
    else:
        assert world == 1, "config {} is a single-GPU run".format(args.config)
        res = run_api(args, dev)
    elapsed = res["elapsed"]
    dist_world, comm_backend = 1, None
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
        dist_world = dist.get_world_size()
        comm_backend = "rccl" if dist.get_backend() == "nccl" else dist.get_backend()
    if rank == 0:
        steps = res.get("steps", args.steps)
        value = res["cells"] * steps / elapsed
        config = {"workload": res["workload"]}
        config.update(res["config"])
        config.update({"decomposition": "slab x{}".format(world) if world > 1 else "none", "rccl_ranks": dist_world,
                       "comm_backend": comm_backend, "exchanges_per_epoch": res["exchanges_per_epoch"]})
        out = {
            "metric": res["metric"], "value": value, "unit": "grid-point-updates/s", "n_gpus": world, "steps": steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": res["dtype"], "data": "synthetic", "config": config,
            "roofline": res["roofline"],
        }
        if res["abytes"]:
            out["epoch_roofline"] = {
                "algorithmic_bytes_per_update": res["abytes"], "achieved": value * res["abytes"] / world / 1e9,
                "frac": value * res["abytes"] / world / 1e9 / HBM_PEAK_GBS, "unit": "GB/s per GPU (SURVEY 8(d) model bytes)",
            }
        out["kernel_ms"] = res["kernel_ms"]
        out["loss_after"] = res["loss"]
        out["full"] = args.full
        parity = check_parity(args, res, world) if args.full else None
        oracle = res.get("oracle")
        if oracle is not None:
            oracle.pop("_fx", None)
        if args.full:
            # N = 1 at the headline size: parity_ok is the VALUE-level comparison with the C oracle's epochs (the emulated-rank
            # table, produced by these same kernels, stays as the trajectory check of N > 1 and is reported beside it)
            ok = [p["ok"] for p in (parity, oracle) if p is not None and p.get("ok") is not None and (p is not oracle or "epochs" in p)]
            out["parity_ok"] = all(ok) if ok else None
            out["parity"] = parity
            out["parity_oracle"] = oracle
        if cpu is not None:
            out["cpu_baseline"] = cpu
        if others is not None:
            out["other_configs"] = others
        out["spinup_ms"] = args.spinup_ms
        if res.get("dumped") is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": res["dumped"]}
        print(json.dumps(out))
        failed = (parity is not None and not parity["ok"]) or (oracle is not None and oracle.get("ok") is False)
    else:
        failed = False
    if world > 1:
        dist.destroy_process_group()
    if failed:
        if parity is None or parity["ok"]:
            sys.exit("bench.py: the first epochs differ from the C oracle's at 512^3: {}".format(oracle))
        sys.exit("bench.py: loss {} after {} epochs differs from the emulated-rank reference {} (rel {:.2e})".format(
            res["loss"], parity["epoch"], parity["expected"], parity["rel_err"]))


if __name__ == "__main__":
    main()
