"""Driver loops and run-time bookkeeping (reference src/odil/util.py).

On the hot path: `optimize_grad` (util.py:190-240), `optimize_newton` (util.py:152-187),
`optimize` (util.py:243-246).  Kept as thin Python host code like the reference; the
difference is that nothing is pulled to the host per epoch: `pinfo` converts its device
scalars lazily, only when a callback actually reads them (the reference's
`np.array(loss)` in core.py:1238-1240 is a device->host sync every epoch).
`make_callback` / `setup_outdir` / `add_arguments` keep the reference's flag names,
`pinfo` keys and the throughput formula (util.py:408-419); history / plotting / checkpoint
file formats are outside the hot path.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from . import gmg, ops
from .core import Field
from .history import History
from .optimizer import EarlyStopError, Optimizer, make_optimizer  # noqa: F401

# Log sink of `printlog` (the reference's module-level names: examples and tests assign them, reference util.py:13-36)
g_log_file = sys.stderr
g_log_echo = False


def assert_equal(first, second, msg=""):
    """ValueError with the reference's wording when the two values differ (reference util.py:15-17)."""
    if first == second:
        return
    raise ValueError("Expected equal '{:}' and '{:}'{}".format(first, second, msg))


def set_log_file(f=None, echo=None):
    """Redirects `printlog` to the open file `f`; `echo` also copies every line to stderr."""
    global g_log_file, g_log_echo
    g_log_file = g_log_file if f is None else f
    g_log_echo = g_log_echo if echo is None else echo


def printlog(*msg):
    """One line, space-separated like print(), to the log file (and to stderr when echoing), flushed at once so
    that `tail -f train.log` follows a run."""
    line = " ".join(str(part) for part in msg) + "\n"
    sinks = [g_log_file]
    if g_log_echo and g_log_file is not sys.stderr:
        sinks.insert(0, sys.stderr)
    for sink in sinks:
        sink.write(line)
        sink.flush()


class LazyPinfo(dict):
    """pinfo = {terms, names, norms, loss} whose device scalars become NumPy on first read."""

    @staticmethod
    def _conv(v):
        if isinstance(v, torch.Tensor):
            return np.array(v.detach().cpu().numpy())
        if isinstance(v, list):
            return [LazyPinfo._conv(a) for a in v]
        return v

    def __getitem__(self, key):
        v = LazyPinfo._conv(dict.__getitem__(self, key))
        dict.__setitem__(self, key, v)
        return v

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]


# --------------------------------------------------------------------------------------
# Arguments: same flag names / defaults as reference util.py:70-149
# --------------------------------------------------------------------------------------
_ARGS = [
    ("--epochs", int, None, "Maximum epochs, defaults to product of plot_every and frames"),
    ("--every_factor", float, 1, "Multiplier for all *_every options"),
    ("--plot_every", int, 5, "Epochs between plots"),
    ("--report_every", int, 10, "Epochs between reports to stdout"),
    ("--history_every", int, 1, "Epochs between entries of training history"),
    ("--checkpoint_every", int, 0, "Epochs between checkpoints"),
    ("--frames", int, 10, "Frames to plot. Zero disables first frame."),
    ("--outdir", str, ".", "Output directory"),
    ("--optimizer", str, "adamn", "Optimizer"),
    ("--seed", int, 1000, "Seed for numpy.random and the backend"),
    ("--plot_title", int, 0, "Enable title in plots"),
    ("--plotext", str, "pdf", "Extension of plots"),
    ("--history_full", int, 0, "Number of epochs to write history at every point"),
    ("--montage", int, 1, "Run montage after plotting"),
    ("--double", int, None, "Double precision. Defaults to runtime.dtype"),
    ("--echo", int, 0, "Echo log to stderr"),
    ("--epoch_start", int, 0, "Initial value of epoch"),
    ("--frame_start", int, 0, "Initial value of frame"),
    ("--checkpoint", str, None, "Continue from checkpoint in state_*.pickle"),
    ("--checkpoint_train", str, None, "Continue from history in state_*_train.pickle"),
    ("--callback_update_state", int, 0, "Update state after callback"),
    ("--bfgs_m", int, 50, "History size for L-BFGS"),
    ("--bfgs_maxls", int, 50, "Max evaluations in line search"),
    ("--bfgs_pgtol", float, None, "Convergence tolerance for L-BFGS-B"),
    ("--adam_epsilon", float, None, "Parameter epsilon in Adam"),
    ("--adam_beta_1", float, None, "Parameter beta_1 in Adam"),
    ("--adam_beta_2", float, None, "Parameter beta_2 in Adam"),
    ("--multigrid", int, 0, "Use multigrid decomposition"),
    ("--dump_data", int, 1, "Dump data_*.pickle with every plot"),
    ("--jac_nsmp0", int, 50, "(unused) Jacobi optimizer option"),
    ("--jac_nsmp1", int, 1, "(unused) Jacobi optimizer option"),
    ("--jac_factor", float, 1, "(unused) Jacobi optimizer option"),
    ("--jac_epsilon", float, 1e-8, "(unused) Jacobi optimizer option"),
]


def add_arguments(parser):
    for flag, typ, default, hlp in _ARGS:
        parser.add_argument(flag, type=typ, default=default, help=hlp)
    parser.add_argument("--mg_interp", type=str, default="stack", choices=["conv", "stack"],
                        help="Multigrid interpolation method (both run the same HIP kernel)")
    parser.add_argument("--nn_initializer", type=str, default="legacy", choices=["legacy", "glorot", "lecun", "he"],
                        help="Initializer for weights of neural networks")


def setup_outdir(args, relpath_args=None):
    """Output directory, args.json, train.log, epoch bookkeeping, seeds (reference util.py:281-334)."""
    from . import runtime

    outdir = args.outdir
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "args.json"), "w") as f:
        env = {k: os.environ.get(k, "") for k in ["ODIL_BACKEND", "ODIL_JIT", "ODIL_MT", "ODIL_DTYPE", "ODIL_FUSE"]}
        d = dict(vars(args), **env, runtime_backend=runtime.backend_name, runtime_dtype=runtime.dtype_name,
                 runtime_jit=runtime.enable_jit, runtime_gpu=True)
        json.dump(d, f, sort_keys=True, indent=4, default=str)
    os.chdir(outdir)
    set_log_file(open("train.log", "w"), echo=args.echo)
    for k in relpath_args or []:
        if getattr(args, k):
            setattr(args, k, os.path.relpath(getattr(args, k), start=outdir))

    # the three cadences are given for every_factor = 1: stretched together, never below one epoch
    for cadence in ("plot_every", "history_every", "report_every"):
        value = getattr(args, cadence)
        if value is not None:
            setattr(args, cadence, max(1, round(value * args.every_factor)))
    if args.epochs is None:  # as many epochs as the requested number of frames needs
        args.epochs = args.frames * args.plot_every
    if args.seed is not None:
        np.random.seed(args.seed)
        runtime.get_mod().random.set_seed(args.seed)
    printlog(" ".join(sys.argv))


def get_memory_usage_kb():
    """Peak resident set size of this process (kB), as the reference reports it (util.py:41-55)."""
    import resource

    return int(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)


def get_gpu_memory_usage_kb():
    """(allocated, reserved) device memory of the caching allocator in kB."""
    if not torch.cuda.is_available():
        return 0, 0
    return torch.cuda.memory_allocated() // 1024, torch.cuda.memory_reserved() // 1024


def make_callback(problem, args=None, epoch_func=None, report_func=None, history_func=None, checkpoint_func=None,
                  plot_func=None):
    cbinfo = argparse.Namespace()
    cbinfo.walltime = 0
    cbinfo.epoch = 0
    cbinfo.time_callback = 0
    cbinfo.time_start = time.time()
    cbinfo.problem = problem
    cbinfo.args = args
    cbinfo.frame = 0
    cbinfo.history = History(csvpath="train.csv", warmup=1) if getattr(args, "history_every", 0) else None

    def callback(state, epoch, pinfo):
        args = cbinfo.args
        domain = problem.domain
        report = bool(args.report_every) and epoch % args.report_every == 0
        hist = cbinfo.history is not None and (epoch % args.history_every == 0 or epoch < (args.history_full or 0))
        plot = epoch % args.plot_every == 0 and bool(epoch or args.frames)
        checkpoint = bool(args.checkpoint_every) and epoch % args.checkpoint_every == 0
        if (report or hist or plot or checkpoint) and torch.cuda.is_available():
            # epochs are enqueued asynchronously (whole epochs as graph replays): wait for the device
            # BEFORE the callback clock starts, so that device time is attributed to the epochs
            torch.cuda.synchronize()
        t_in = time.time()
        cbinfo.task_report, cbinfo.task_history, cbinfo.task_plot, cbinfo.task_checkpoint = report, hist, plot, checkpoint
        cbinfo.pinfo = pinfo
        if isinstance(problem.tracers, dict):
            problem.tracers["epoch"] = epoch
        if epoch_func is not None:
            epoch_func(problem, state, epoch, cbinfo)
        now = time.time()
        cbinfo.time_callback += now - t_in
        t_in = now
        walltime = now - cbinfo.time_start - cbinfo.time_callback
        if report:
            printlog("\nepoch={:05d}".format(epoch))
            if pinfo and "norms" in pinfo:
                norms, names = pinfo["norms"], pinfo["names"]
                printlog("residual: " + ", ".join(
                    "{}:{:.5g}".format(name or str(i), float(np.array(norm)))
                    for i, (norm, name) in enumerate(zip(norms, names))))
            if report_func is not None:
                report_func(problem, state, epoch, cbinfo)
            if epoch > cbinfo.epoch:
                wte = (walltime - cbinfo.walltime) / (epoch - cbinfo.epoch)
                thr = np.prod(domain.cshape) / wte if wte > 0 else 0
            else:
                wte, thr = 0, 0
            gpu_used, gpu_pool = get_gpu_memory_usage_kb()
            printlog("memory: {:} MiB, gpu_used: {:} MiB, gpu_pool: {:} MiB".format(
                get_memory_usage_kb() // 1024, gpu_used // 1024, gpu_pool // 1024))
            printlog("walltime: {:.3f} s, walltime+callback: {:.3f} s, walltime/epoch: {:.3f} ms".format(
                walltime, walltime + cbinfo.time_callback, wte * 1000))
            printlog("throughput: {:.3f} Mcells/s".format(thr / 1e6))
            cbinfo.walltime, cbinfo.epoch = walltime, epoch
        if hist:
            h = cbinfo.history
            h.append("epoch", epoch)
            h.append("frame", cbinfo.frame)
            if pinfo and "norms" in pinfo:
                for i, (norm, name) in enumerate(zip(pinfo["norms"], pinfo["names"])):
                    h.append("norm_{:}".format(name or str(i)), np.array(norm))
            if pinfo and "loss" in pinfo:
                h.append("loss", np.array(pinfo["loss"]))
            if getattr(args, "linsolver_history", 0) and pinfo and "linsolver" in pinfo:
                for key, val in pinfo["linsolver"].items():
                    if isinstance(val, (int, float, str, np.floating)):
                        h.append("lin_" + key, val)
            h.append("walltime", float(np.round(walltime, 3)))
            gpu_used, gpu_pool = get_gpu_memory_usage_kb()
            h.append("memory", get_memory_usage_kb() // 1024)
            h.append("gpu_used", gpu_used // 1024)
            h.append("gpu_pool", gpu_pool // 1024)
            if history_func is not None:
                history_func(problem, state, epoch, h, cbinfo)
            h.write()
        if plot:
            if plot_func is not None:
                plot_func(problem, state, epoch, cbinfo.frame, cbinfo)
            cbinfo.frame += 1
        if checkpoint:
            if checkpoint_func is not None:
                checkpoint_func(problem, state, epoch, cbinfo)
            else:
                from .core import checkpoint_save

                path = "checkpoint_{:06d}.pickle".format(epoch)
                printlog(path)
                checkpoint_save(domain, state, path)
        cbinfo.time_callback += time.time() - t_in

    def next_active(epoch):
        """The first epoch after `epoch` at which this callback does anything (report, history, plot, checkpoint, a user
        hook): on the epochs before it a call is a no-op, so an optimizer may run them without calling."""
        args = cbinfo.args
        if epoch_func is not None:
            return epoch + 1
        e = epoch + 1
        while True:
            if ((bool(args.report_every) and e % args.report_every == 0)
                    or (cbinfo.history is not None and (e % args.history_every == 0 or e < (args.history_full or 0)))
                    or (e % args.plot_every == 0 and bool(e or args.frames))
                    or (bool(args.checkpoint_every) and e % args.checkpoint_every == 0)):
                return e
            e += 1

    callback.cbinfo = cbinfo
    callback.next_active = next_active
    return callback


# --------------------------------------------------------------------------------------
# Driver loops
# --------------------------------------------------------------------------------------
def _pinfo(loss, terms, names, norms):
    return LazyPinfo(terms=terms, names=names, norms=norms, loss=loss)


def _poisson_newton_step(problem, state, args, status):
    """Newton step of a problem already recognised as the Poisson stencil (fused.detect: f(u) = A u -
    rhs with the zero-Dirichlet Laplacian A): d with A d = f(u) straight from the fused residual and the
    geometric multigrid, without forming the seven coefficient arrays of the Jacobian and without
    re-recognising them (512^3: 75 ms of a 215 ms step).  None when the general route must be taken:
    other operators, multigrid-decomposed unknowns, or a request the constant-coefficient cycles of linsolver.ROUTES
    do not take (the same helpers decide here and there).  d may be a work buffer of the solver."""
    from . import linsolver as ls

    if state.initialized:
        problem.recognise(state)  # (without a callback no evaluation precedes the first step)
    ev = getattr(problem, "_fused", None)
    if ev is None or ev.nlvl != 1 or len(state.fields) != 1 or not int(os.environ.get("ODIL_NEWTON_SHORTCUT", 1)):
        return None  # (ODIL_NEWTON_SHORTCUT=0: the general route eval_operator_grad -> linearize -> linsolver.solve)
    (field,) = state.fields.values()
    damped = getattr(args, "linsolver_damp", 0) or getattr(args, "linsolver_dampdiag", 0)
    linsolver = getattr(args, "linsolver", "direct")
    if not isinstance(field, Field) or not ls.cycles_apply(linsolver, field.array.numel(), damped):
        return None
    r, _ = ops.poisson_residual(field.array.contiguous(), ev.rhs, ev.h2, fu=ev.fu, loss=ev.loss)
    tol, maxiter = ls.cycle_budget(linsolver, getattr(args, "linsolver_tol", 1e-10), getattr(args, "linsolver_maxiter", None))
    mixed = ls.gmg_mixed(ev.dtype, ev.cshape)
    solver = ls.poisson_gmg(problem.domain, ev.cshape, ev.h2, ev.dtype, ev.device, mixed=mixed)
    if mixed:
        return gmg.solve_mixed(solver[0], solver[1], r, tol=tol, maxiter=maxiter, status=status).reshape(-1)
    # (||r||: the evaluation above reduced mean(r^2) into ev.loss already)
    return solver.solve(r, tol=tol, maxiter=maxiter, status=status, copy=False, b_meansq=ev.loss).reshape(-1)


def optimize_newton(args, problem, state, callback=None, **kwargs):
    """x <- x + delta with (M^T M) delta = -M^T r per epoch (reference util.py:152-187)."""
    from .linsolver import solve

    domain = problem.domain

    def eval_pinfo(state):
        loss, _, terms, names, norms = problem.eval_loss_grad_device(state)
        return _pinfo(loss, terms, names, norms)

    opt = Optimizer(name="newton", displayname="Newton")
    printlog("Running {} optimizer".format(opt.displayname))
    if callback:  # (the evaluations around the steps exist for the report only, reference util.py:156-158, 180)
        callback(state, args.epoch_start, eval_pinfo(state))
    for epoch in range(args.epoch_start, args.epochs):
        opt.evals += 1
        linstatus = dict()
        # Every route returns d with M d = r, and x - d is formed here: each is a linear solve, whose result for -r is
        # exactly -d (IEEE arithmetic is symmetric in sign) -- no pass that negates r first; d is consumed before the next
        # solve (no copy out of the solver's work buffers)
        d = _poisson_newton_step(problem, state, args, linstatus)
        if d is None:
            vector, matrix = problem.linearize_device(state)
            d = solve(matrix, vector.contiguous(), args, linstatus, getattr(args, "linsolver", "direct"), consume=True)
        if getattr(args, "linsolver_verbose", 0):
            printlog(linstatus)
        fields = list(state.fields.values())
        if len(fields) == 1 and type(fields[0]) is Field and torch.is_tensor(fields[0].array) \
                and fields[0].array.is_contiguous() and fields[0].array.numel() == d.numel():
            ops.axpy(fields[0].array, d.to(fields[0].array.dtype), -1.0)  # x -= d in place (util.py:176-178)
        else:
            domain.unpack_state(domain.pack_state(state) - d, state)
        if callback:  # one extra evaluation per step, for the report only (reference util.py:180)
            report = eval_pinfo(state)
            report["linsolver"] = linstatus
            callback(state, epoch + 1, report)
    return domain.arrays_from_state(state), argparse.Namespace(epochs=args.epochs, evals=args.epochs)


def make_loss_grad(problem, state):
    """The `loss_grad(arrays) -> (loss, grads, pinfo)` callable the optimizers drive (reference util.py:197-206),
    with this package's hooks attached: `fused_adam` (update inside the gradient launches), `graph_safe` /
    `graph_begin` / `refresh` / `graph_end` (epochs replayed as a hipGraph)."""
    domain = problem.domain

    def loss_grad(arrays):
        domain.arrays_to_state(arrays, state)
        loss, grads, terms, names, norms = problem.eval_loss_grad_device(state)
        return loss, grads, _pinfo(loss, terms, names, norms)

    def fused_adam(arrays, m, v, alpha, omb1, omb2, eps):
        """loss + gradient with the Adam update of the leading array(s) applied inside the fused
        gradient launch; None when the problem has no fused evaluator that can do it."""
        ev = getattr(problem, "_fused", None) or getattr(problem, "_traced", None)
        if ev is None or not hasattr(ev, "eval_loss_grad_adam"):
            return None
        domain.arrays_to_state(arrays, state)
        res = ev.eval_loss_grad_adam(state, m, v, alpha, omb1, omb2, eps)
        if res is None:
            return None
        loss, grads, terms, names, norms, done = res
        return loss, grads, _pinfo(loss, terms, names, norms), done

    def small_epochs(arrays, m, v, table, omb1, omb2, eps):
        """A runner of whole Adam epochs in ONE launch each call (small 1-D / 2-D Poisson problems,
        fused.PoissonEvaluator.small_epochs), or None when the problem is not of that kind.  `table`: device tensor of
        the run's step sizes; runner(first, count) runs the epochs that use table[first : first + count] and returns the
        report of the last of them (device scalars, read lazily)."""
        ev = getattr(problem, "_fused", None)
        if ev is None or not hasattr(ev, "small_plan"):
            return None
        heads = ev.small_plan(arrays, m, v)
        if heads is None:
            return None
        domain.arrays_to_state(arrays, state)
        losses, norms = torch.empty_like(table), torch.empty_like(table)

        def runner(first, count):
            ev.small_epochs(heads, table[first:first + count], losses[first:first + count], norms[first:first + count],
                            omb1, omb2, eps)
            k = first + count - 1
            return _pinfo(losses[k], [losses[k]], ev.names, [norms[k]])

        return runner

    loss_grad.fused_adam = fused_adam
    loss_grad.small_epochs = small_epochs
    # hipGraph replay of whole Adam epochs (optimizer._EpochGraph): possible when the evaluation is
    # made of this package's kernels only -- the generic path has its own graph (Problem(jit=True))
    # (outputs in parameter space: replayable when they run as the generated kernel of param_expr.py; the torch replay
    # of param_tape.py bakes the host scalars of the current epoch in)
    loss_grad.graph_safe = lambda: getattr(problem, "_fused", None) is not None or (
        getattr(problem, "_traced", None) is not None and getattr(problem._traced, "graph_ok", True) and (
            not getattr(problem._traced, "offgrid", None) or getattr(problem._traced, "par_outputs", None) is not None))

    def graph_hook(name):
        def call(*a):
            traced = getattr(problem, "_traced", None)
            if traced is not None:
                getattr(traced, name)(*a)

        return call

    # replayed epochs: host scalars of a traced operator travel as rows of a device table (stencil_jit.py)
    loss_grad.graph_begin, loss_grad.refresh, loss_grad.graph_end = (
        graph_hook("graph_begin"), graph_hook("graph_upload"), graph_hook("graph_end"))
    return loss_grad


def optimize_grad(args, optname, problem, state, callback=None, **kwargs):
    """Gradient-based optimisation (reference util.py:190-240)."""
    domain = problem.domain
    mod = domain.mod
    loss_grad = make_loss_grad(problem, state)

    def callback_wrap(arrays, epoch, pinfo):
        domain.arrays_to_state(arrays, state)
        callback(state, epoch, pinfo)
        if getattr(args, "callback_update_state", 0):
            new = domain.arrays_from_state(state)
            for i in range(len(new)):
                arrays[i] = new[i]

    # (a callback that tells when it next DOES something lets the optimizer run the epochs in between in one launch)
    if not getattr(args, "callback_update_state", 0):
        callback_wrap.next_active = getattr(callback, "next_active", None)

    for src, dst in [("bfgs_m", "m"), ("bfgs_pgtol", "pgtol"), ("bfgs_maxls", "maxls"), ("adam_epsilon", "epsilon"),
                     ("adam_beta_1", "beta_1"), ("adam_beta_2", "beta_2")]:
        if getattr(args, src, None) is not None:
            kwargs[dst] = getattr(args, src)
    opt = make_optimizer(optname, dtype=domain.dtype, mod=mod, **kwargs)
    printlog("Running {} optimizer".format(opt.displayname))
    arrays = domain.arrays_from_state(state)
    _, _, pinfo = loss_grad(arrays)
    if callback:
        callback(state, args.epoch_start, pinfo)
    arrays, optinfo = opt.run(
        arrays, loss_grad=loss_grad, epochs=args.epochs - args.epoch_start,
        callback=callback_wrap if callback else None, epoch_start=args.epoch_start, lr=args.lr, **kwargs,
    )
    domain.arrays_to_state(arrays, state)
    return arrays, optinfo


def optimize_ensemble(args, problems, states, callback=None, lrs=None, form="workgroup", **kwargs):
    """Adam on B small Poisson problems AT ONCE: every launch runs whole epochs of all members, one workgroup per member
    (fused.PoissonEnsemble; a sweep over right-hand sides, initial guesses or step sizes of a problem that alone fills
    1 / 256 of the device).  Every member ends where `optimize_grad(args, "adam", problem, state)` would leave it, bit for bit.

    form: 'workgroup' (the default) is the above.  'launches' runs members of ANY 1-D / 2-D size with at least two levels
    (fused.PoissonLaunchEnsemble, fused.launches_refusal): every epoch is the launches of a single run, each covering all
    members.  'volumes' runs 3-D members with at least two levels the same way (fused.PoissonVolumeEnsemble,
    fused.volumes_refusal).  'auto': 'volumes' for 3-D members; else 'workgroup' where `fused.small_refusal` admits the
    members, 'launches' otherwise.

    args.optimizer must be 'adam' / 'adamn'; lrs: one step size per member (default args.lr for all).
    callback(member, state, epoch, pinfo): called for every member at args.epoch_start (the initial evaluation) and at
    the epochs its `next_active(epoch)` attribute names (the cadence of `make_callback`; without the attribute: every
    epoch), pinfo as `optimize_grad` reports it, device scalars read lazily.  The callback reads the state; arrays it
    swaps in are not picked up.
    Members must be the recognised Poisson operator, share cshape, level shapes, spacing, dtype and device, and be
    admitted by the form that runs them (fused.small_refusal: small enough for the one-workgroup epochs;
    fused.launches_refusal: 1-D / 2-D, at least two levels that halve; fused.volumes_refusal: 3-D, at least two levels
    that halve, a finest extent of at least 4); anything else raises ValueError naming the first
    offending member -- structure (shapes, size) is checked for all members before any operator is probed.
    Returns ([level arrays of member b], optinfo); optinfo.losses / .norms: [B, epochs] device tensors."""
    from . import fused

    optname = getattr(args, "optimizer", "adam")
    if optname not in ("adam", "adamn"):
        raise ValueError("optimize_ensemble runs Adam ('adam' / 'adamn'), not optimizer '{}'".format(optname))
    if not problems or len(problems) != len(states):
        raise ValueError("optimize_ensemble: {} problems with {} states".format(len(problems), len(states)))
    if lrs is not None and len(lrs) != len(problems):
        raise ValueError("optimize_ensemble: {} step sizes for {} members".format(len(lrs), len(problems)))

    def refuse(member, reason):
        raise ValueError("optimize_ensemble: member {}: {}".format(member, reason))

    fused.ensemble_form(form, [(2,)], torch.float64)  # (any other value of `form` raises here)
    first = None
    for b, (problem, state) in enumerate(zip(problems, states)):
        domain = problem.domain
        if not state.initialized:
            refuse(b, "uninitialized state, use `state = domain.init_state(state)`")
        if len(state.fields) != 1:
            refuse(b, "{} unknown fields (the Poisson problem has one)".format(len(state.fields)))
        arrays = domain.arrays_from_state(state)
        shapes = [tuple(int(n) for n in a.shape) for a in arrays]
        if shapes[0] != tuple(domain.cshape):
            refuse(b, "the unknown is not a cell-centred field of the domain")
        if b == 0:
            form = fused.ensemble_form(form, shapes, arrays[0].dtype)
        predicate = dict(workgroup=fused.small_refusal, launches=fused.launches_refusal, volumes=fused.volumes_refusal)[form]
        reason = predicate(shapes, arrays[0].dtype)
        if reason is not None:
            refuse(b, reason)
        kind = dict(shapes=shapes, dtype=arrays[0].dtype, device=arrays[0].device,
                    spacing=[float(domain.step_by_dim(i)) for i in range(domain.ndim)])
        first = first or kind
        for what, label in (("shapes", "level shapes"), ("dtype", "dtype"), ("device", "device"), ("spacing", "grid spacing")):
            if kind[what] != first[what]:
                refuse(b, "{} {} differ from member 0's {}".format(label, kind[what], first[what]))
    evaluators = []
    for b, (problem, state) in enumerate(zip(problems, states)):
        problem.recognise(state)
        if getattr(problem, "_fused", None) is None:
            refuse(b, "the operator is not the recognised Poisson stencil")
        evaluators.append(problem._fused)
    kind = dict(workgroup=fused.PoissonEnsemble, launches=fused.PoissonLaunchEnsemble, volumes=fused.PoissonVolumeEnsemble)[form]
    reason = kind.refusal(evaluators)
    if reason is not None:
        refuse(*reason)
    ensemble = kind(evaluators)
    for b, (problem, state) in enumerate(zip(problems, states)):
        levels = ensemble.levels(ensemble.x, b)
        for dst, src in zip(levels, problem.domain.arrays_from_state(state)):
            dst.copy_(src)
        problem.domain.arrays_to_state(levels, state)  # (views of the packed state: always the current iterate)

    for src, dst in [("adam_epsilon", "epsilon"), ("adam_beta_1", "beta_1"), ("adam_beta_2", "beta_2")]:
        if getattr(args, src, None) is not None:
            kwargs[dst] = getattr(args, src)
    opt = make_optimizer(optname, dtype=problems[0].domain.dtype, mod=problems[0].domain.mod)
    printlog("Running {} optimizer on an ensemble of {} members".format(opt.displayname, len(problems)))

    def callback_wrap(epoch, losses, norms):
        for b, (problem, state) in enumerate(zip(problems, states)):
            callback(b, state, epoch, _pinfo(losses[b], [losses[b]], ensemble.names[b], [norms[b]]))

    if callback:
        callback_wrap.next_active = getattr(callback, "next_active", None)
        for b, (problem, state) in enumerate(zip(problems, states)):  # (the report of the start, as optimize_grad makes it)
            loss, _, terms, names, norms = problem.eval_loss_grad_device(state)
            callback(b, state, args.epoch_start, _pinfo(loss, terms, names, norms))
    return opt.run_ensemble(ensemble, epochs=args.epochs - args.epoch_start, callback=callback_wrap if callback else None,
                            lr=args.lr, lrs=lrs, epoch_start=args.epoch_start, **kwargs)


def optimize_newton_ensemble(args, problems, states, callback=None):
    """Newton on B small Poisson problems AT ONCE: every epoch is ONE launch that runs the whole Newton step of all
    members, one workgroup per member (gmg.EnsembleGMG.newton_step: residual, nested-iteration start, V-cycles down to the
    tolerance, the convergence decision and the update, no host read-back in between).  Every member ends at the Newton
    iterate `optimize_newton(args, problem, state)` reaches for it alone, to the tolerance of the linear solve.

    args.linsolver must be 'direct' or 'multigrid', without damping; tolerance and cycle budget are those of the
    single-problem multigrid route (linsolver.cycle_budget, at least 50 eps of the working precision).
    callback(member, state, epoch, pinfo): called for every member at args.epoch_start (the initial evaluation) and at the
    epochs its `next_active(epoch)` attribute names (without the attribute: every epoch); pinfo as `optimize_newton`
    reports it, after a step with pinfo["linsolver"] = the member's solver status.
    Members have one plain `Field` unknown (no multigrid decomposition), are the recognised Poisson operator (else below), share
    cshape, spacing, dtype and device and be admitted by `fused.newton_refusal`; anything else raises ValueError naming the
    first offending member -- structure is checked for all members before any operator is probed.

    When not every member is that Poisson operator, ALL members take the route for variable-coefficient stencils
    (optinfo.route == "stencil", and `solver.method` says so): any operator of one plain cell-centred `Field` whose Jacobian
    is a (2 d + 1)-point stencil -- variable conductivities, reaction and nonlinear terms -- admitted by
    `fused.newton_stencil_refusal`, same cshape, spacing, dtype and device.  Per epoch: every member is linearised
    (`linearize_device`, `gmg.recognise_stencil`: B launches of the generated Jacobian kernel -- a batched one would be a
    change of the generator), the coefficient arrays and f(u) go into packed buffers allocated once, the hierarchies of all
    members are set up again in launches that do not grow with B (`gmg.EnsembleGMG.rebuild`: two per level, one for the
    dense coarsest matrices; the pseudo-inverses on the host), ONE launch solves M_b d_b = f_b(u_b) for all members and one
    forms u -= d.  A member whose Jacobian is no such stencil raises ValueError naming it at the first epoch, before any
    member is updated; so do members whose hierarchies do not coarsen along the same axes.  There is NO fallback to the
    normal-equation routes when a member's cycles do not contract (`optimize_newton` has one): the member's status
    reports converged=False or stagnated, and the caller decides.
    Returns ([arrays of member b], optinfo); optinfo.cycles / .residuals: [B, epochs] cycles run and final residual norms;
    optinfo.route: "poisson" or "stencil"."""
    from . import fused
    from . import linsolver as ls

    if not problems or len(problems) != len(states):
        raise ValueError("optimize_newton_ensemble: {} problems with {} states".format(len(problems), len(states)))
    linsolver = getattr(args, "linsolver", "direct")
    if linsolver not in ("direct", "multigrid"):
        raise ValueError("optimize_newton_ensemble: linsolver '{}' (the one-workgroup Newton solves serve 'direct' and "
                         "'multigrid')".format(linsolver))
    if getattr(args, "linsolver_damp", 0) or getattr(args, "linsolver_dampdiag", 0):
        raise ValueError("optimize_newton_ensemble: damping (linsolver_damp / linsolver_dampdiag) is not served: the cycles "
                         "solve M d = r, which has the solution of the normal equations only without it")

    def refuse(member, reason):
        raise ValueError("optimize_newton_ensemble: member {}: {}".format(member, reason))

    routes = dict(poisson=None, stencil=None)  # per route the first (member, reason) it refuses while the other admits
    first = None
    for b, (problem, state) in enumerate(zip(problems, states)):
        domain = problem.domain
        if not state.initialized:
            refuse(b, "uninitialized state, use `state = domain.init_state(state)`")
        if len(state.fields) != 1:
            refuse(b, "{} unknown fields (the Poisson problem has one)".format(len(state.fields)))
        (field,) = state.fields.values()
        if type(field) is not Field:
            refuse(b, "the unknown is a {} (a plain Field is needed: no multigrid decomposition)".format(type(field).__name__))
        cshape = tuple(int(n) for n in domain.cshape)
        if tuple(int(n) for n in field.array.shape) != cshape or field.loc != "c" * domain.ndim:
            refuse(b, "the unknown is not a cell-centred field of the domain")
        dtype = field.array.dtype
        npdt = np.float64 if dtype == torch.float64 else np.float32
        kind = dict(cshape=cshape, dtype=dtype, device=field.array.device,
                    spacing=[float(domain.step_by_dim(i)) for i in range(domain.ndim)])
        # (which route runs is known only once the operators are probed: a member that neither admits is refused here, one
        # that a single route refuses once the route is known -- still before any state changes)
        reason = fused.newton_refusal(cshape, [npdt(v) ** 2 for v in kind["spacing"]], dtype)
        other = fused.newton_stencil_refusal(cshape, dtype)
        if reason is not None and other is not None:
            refuse(b, reason)
        if reason is not None and routes["poisson"] is None:
            routes["poisson"] = (b, reason)
        if other is not None and routes["stencil"] is None:
            routes["stencil"] = (b, other)
        first = first or kind
        for what, label in (("cshape", "cells"), ("dtype", "dtype"), ("device", "device"), ("spacing", "grid spacing")):
            if kind[what] != first[what]:
                refuse(b, "{} {} differ from member 0's {}".format(label, kind[what], first[what]))
    evaluators = []
    for b, (problem, state) in enumerate(zip(problems, states)):
        problem.recognise(state)
        ev = getattr(problem, "_fused", None)
        evaluators.append(ev if ev is not None and ev.nlvl == 1 else None)
    if any(ev is None for ev in evaluators):
        if routes["stencil"] is not None:
            refuse(*routes["stencil"])
        return _newton_ensemble_stencil(args, problems, states, callback, first, linsolver)
    if routes["poisson"] is not None:
        refuse(*routes["poisson"])
    ev = evaluators[0]
    nb = len(problems)
    solver = gmg.EnsembleGMG(ev.cshape, ev.h2, ev.dtype, ev.device, nb)
    u = torch.stack([problem.domain.arrays_from_state(state)[0].to(ev.dtype) for problem, state in zip(problems, states)])
    rhs = torch.stack([e.rhs.reshape(ev.cshape) for e in evaluators])
    for b, (problem, state) in enumerate(zip(problems, states)):
        problem.domain.arrays_to_state([u[b]], state)  # (views of the packed iterate: always the current one)
    tol, maxcycles = ls.cycle_budget(linsolver, getattr(args, "linsolver_tol", 1e-10), getattr(args, "linsolver_maxiter", None))
    tol = max(tol, 50 * float(torch.finfo(ev.dtype).eps))
    printlog("Running Newton optimizer on an ensemble of {} members".format(nb))

    def report(epoch, stepped):
        for b, (problem, state) in enumerate(zip(problems, states)):
            loss, _, terms, names, norms = problem.eval_loss_grad_device(state)
            pinfo = _pinfo(loss, terms, names, norms)
            if stepped:
                pinfo["linsolver"] = solver.status(b)
            callback(b, state, epoch, pinfo)

    nepochs = max(args.epochs - args.epoch_start, 0)
    cycles = np.zeros((nb, nepochs), dtype=np.int64)
    residuals = np.zeros((nb, nepochs))
    next_active = getattr(callback, "next_active", None) if callback else None
    due = None
    if callback:
        report(args.epoch_start, False)
        due = next_active(args.epoch_start) if next_active else args.epoch_start + 1
    for epoch in range(args.epoch_start, args.epochs):
        solver.newton_step(u, rhs, tol=tol, maxcycles=maxcycles)
        k = epoch - args.epoch_start
        cycles[:, k] = solver.outcome[:, 0]
        residuals[:, k] = [solver.status(b)["residual"] for b in range(nb)]
        if getattr(args, "linsolver_verbose", 0):
            printlog([solver.status(b) for b in range(nb)])
        if callback and epoch + 1 >= due:
            report(epoch + 1, True)
            due = next_active(epoch + 1) if next_active else epoch + 2
    arrays = [problem.domain.arrays_from_state(state) for problem, state in zip(problems, states)]
    return arrays, argparse.Namespace(epochs=args.epochs, evals=nepochs, cycles=cycles, residuals=residuals, solver=solver,
                                      route="poisson")


def _newton_ensemble_stencil(args, problems, states, callback, kind, linsolver):
    """The route of `optimize_newton_ensemble` for members that are not all the Poisson operator (its docstring); the
    members have passed its checks, `kind` is what they share."""
    from . import linsolver as ls

    nb, cshape, dtype, device = len(problems), kind["cshape"], kind["dtype"], kind["device"]
    ndim = len(cshape)
    stage = torch.empty((nb, 2 * ndim + 1) + cshape, dtype=dtype, device=device)  # (the Jacobians of the first step)
    r = torch.empty((nb,) + cshape, dtype=dtype, device=device)
    d = torch.zeros_like(r)

    def linearise(target):
        """r[b] = f_b(u_b) and target[b] = the coefficient arrays of member b's Jacobian, for every member."""
        for b, (problem, state) in enumerate(zip(problems, states)):
            vector, matrix = problem.linearize_device(state)
            coeffs = gmg.recognise_stencil(matrix)
            if coeffs is None or tuple(coeffs.shape[1:]) != cshape:
                raise ValueError("optimize_newton_ensemble: member {}: its Jacobian is not a (2 d + 1)-point stencil of one "
                                 "cell-centred plain Field".format(b))
            target[b].copy_(coeffs)
            r[b].view(-1).copy_(vector.reshape(-1))

    nepochs = max(args.epochs - args.epoch_start, 0)
    solver = None
    if nepochs:  # (the first linearisation before anything changes: a member that has no stencil Jacobian is named here)
        linearise(stage)
        solver = gmg.EnsembleGMG.from_coeffs(stage)
    del stage
    u = torch.stack([problem.domain.arrays_from_state(state)[0].to(dtype) for problem, state in zip(problems, states)])
    for b, (problem, state) in enumerate(zip(problems, states)):
        problem.domain.arrays_to_state([u[b]], state)  # (views of the packed iterate: always the current one)
    tol, maxcycles = ls.cycle_budget(linsolver, getattr(args, "linsolver_tol", 1e-10), getattr(args, "linsolver_maxiter", None))
    tol = max(tol, 50 * float(torch.finfo(dtype).eps))
    printlog("Running Newton optimizer on an ensemble of {} members (variable-coefficient stencils)".format(nb))

    def report(epoch, stepped):
        for b, (problem, state) in enumerate(zip(problems, states)):
            loss, _, terms, names, norms = problem.eval_loss_grad_device(state)
            pinfo = _pinfo(loss, terms, names, norms)
            if stepped:
                pinfo["linsolver"] = solver.status(b)
            callback(b, state, epoch, pinfo)

    cycles = np.zeros((nb, nepochs), dtype=np.int64)
    residuals = np.zeros((nb, nepochs))
    next_active = getattr(callback, "next_active", None) if callback else None
    due = None
    if callback:
        report(args.epoch_start, False)
        due = next_active(args.epoch_start) if next_active else args.epoch_start + 1
    for epoch in range(args.epoch_start, args.epochs):
        if epoch > args.epoch_start:
            linearise(solver.fine)
            solver.rebuild()
        solver.solve(r, d, tol=tol, maxcycles=maxcycles, start=2)  # M_b d_b = r_b, the convention of optimize_newton
        ops.axpy(u.view(-1), d.view(-1), -1.0)                     # u -= d for all members
        k = epoch - args.epoch_start
        cycles[:, k] = solver.outcome[:, 0]
        residuals[:, k] = [solver.status(b)["residual"] for b in range(nb)]
        if getattr(args, "linsolver_verbose", 0):
            printlog([solver.status(b) for b in range(nb)])
        if callback and epoch + 1 >= due:
            report(epoch + 1, True)
            due = next_active(epoch + 1) if next_active else epoch + 2
    arrays = [problem.domain.arrays_from_state(state) for problem, state in zip(problems, states)]
    return arrays, argparse.Namespace(epochs=args.epochs, evals=nepochs, cycles=cycles, residuals=residuals, solver=solver,
                                      route="stencil")


def optimize(args, optname, problem, state, callback, **kwargs):
    if optname == "newton":
        return optimize_newton(args, problem, state, callback, **kwargs)
    return optimize_grad(args, optname, problem, state, callback, **kwargs)
