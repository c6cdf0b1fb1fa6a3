"""Newton on the slab decomposition (odil_amd/slab_solvers.py: SlabTracedNewton, slab_traced.optimize_slab with
`--optimizer newton`) against the undivided single-GPU Newton route (`Problem.linearize_device` with the generated `k_jac`,
`gmg.recognise_stencil`, `util.optimize_newton`).  Ranks run as threads on one GPU (`slab_solvers.run_threads`); the
end-to-end case runs two processes over gloo under torch.distributed.run.  Operators: examples/diffusion (smooth and
jumping conductivity, with a reaction term) and a NONLINEAR diffusion div((1 + u^2) grad u) - f, whose coefficients depend
on u across the rank interfaces and the ends of the cut axis (the ghost and wrap inputs of the slab `k_jac`)."""

import argparse
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
sys.path.insert(0, os.path.join(ROOT, "examples", "darcy"))

pytestmark = pytest.mark.gpu

SHAPES = {"cube": (32, 32, 32), "box": (48, 32, 16)}
CASES = [("cube", 2), ("cube", 4), ("box", 2), ("box", 3), ("box", 4)]


@pytest.fixture(autouse=True)
def quiet():
    import odil_amd as odil

    saved = odil.util.g_log_file
    odil.util.set_log_file(open(os.devnull, "w"))
    yield
    odil.util.g_log_file = saved


def nonlinear_operator(ctx):
    """div((1 + u^2) grad u) - f with the quadratic wall ghosts of examples/diffusion (face values of 1 + u^2 averaged)."""
    import odil_amd as odil

    mod, extra = ctx.mod, ctx.extra
    q = ctx.field("u")
    iw, nw, dw = ctx.indices(), ctx.size(), ctx.step()
    zero = mod.cast(0, q.dtype)
    total = None
    for i in range(3):
        qm = ctx.field("u", *[-1 if j == i else 0 for j in range(3)])
        qp = ctx.field("u", *[1 if j == i else 0 for j in range(3)])
        gm = mod.where(iw[i] == 0, odil.core.extrap_quadh(qp, q, zero), qm)
        gp = mod.where(iw[i] == nw[i] - 1, odil.core.extrap_quadh(qm, q, zero), qp)
        km, kp = 1 + 0.5 * (q**2 + gm**2), 1 + 0.5 * (q**2 + gp**2)
        term = (kp * (gp - q) - km * (q - gm)) / dw[i] ** 2
        total = term if total is None else total + term
    return [total - extra.rhs]


def periodic_operator(ctx):
    """A periodic Laplacian minus u (nonsingular): couples across the ends of every axis."""
    total = -ctx.field("u")
    dw = ctx.step()
    for i in range(3):
        qm = ctx.field("u", *[-1 if j == i else 0 for j in range(3)])
        qp = ctx.field("u", *[1 if j == i else 0 for j in range(3)])
        total = total + (qp - 2 * ctx.field("u") + qm) / dw[i] ** 2
    return [total - ctx.extra.rhs]


def make(kind, shape, double=True, sigma=0.0, random=True):
    """(problem, state) on the GPU: examples/diffusion's operator ('smooth', 'jump') on an arbitrary box, or the nonlinear /
    periodic operators above; random=True: a random state (else zeros, Newton's start)."""
    import diffusion as ex

    import odil_amd as odil

    dtype = np.float64 if double else np.float32
    domain = odil.Domain(cshape=list(shape), dimnames=["x", "y", "z"], multigrid=0, dtype=dtype)
    mod = domain.mod
    x1 = [np.asarray(mod.numpy(x), dtype=np.float64) for x in domain.points_1d()]
    xx = np.meshgrid(*x1, indexing="ij")
    rhs = mod.cast(np.sin(np.pi * xx[0]) * np.cos(2 * xx[1]) + xx[2], dtype)
    args = argparse.Namespace(sigma=sigma)
    if kind in ("smooth", "jump"):
        step = [float(s) for s in domain.step()]
        kfaces = []
        for i in range(3):
            pair = []
            for sign in (-0.5, 0.5):
                coords = [x + (sign * step[i] if j == i else 0.0) for j, x in enumerate(x1)]
                pair.append(mod.cast(ex.conductivity(kind, np.meshgrid(*coords, indexing="ij")), dtype))
            kfaces.append(tuple(pair))
        extra = argparse.Namespace(rhs=rhs, kfaces=kfaces, args=args)
        operator = ex.operator
    else:
        extra = argparse.Namespace(rhs=rhs)
        operator = {"nonlinear": nonlinear_operator, "periodic": periodic_operator}[kind]
    state = odil.State()
    state.fields["u"] = None
    state = domain.init_state(state)
    if random:
        rng = np.random.default_rng(11)
        u = torch.tensor(rng.standard_normal(tuple(shape)) * 0.5, dtype=torch.float64).to(domain.mod.device)
        domain.arrays_to_state([u.to(state.fields["u"].array.dtype)], state)
    return odil.Problem(operator, domain, extra), state


def jac_kernels(*a):
    from odil_amd.slab_traced import HipSlabKernels

    return HipSlabKernels(*a, jac=True)


def slab_jacobians(problem, state, world):
    """Per rank: (value, [7, n, N1, N2] coefficients) of the slab `k_jac` at `state`."""
    from odil_amd.gmg import stencil_coefficients
    from odil_amd.slab_solvers import drive, run_threads
    from odil_amd.slab_traced import SlabTracedAdam

    def body(rank, comm):
        run = SlabTracedAdam(problem, state, rank, world, kernels=jac_kernels)
        drive(run.evaluate_gen(), comm)
        buf = run.kern.jacobian(run.u, *run.wrap_planes())
        items = [(attr[1], buf[j]) for j, (_, attr) in enumerate(run.kern.jac_items) if attr is not None]
        value = buf[[attr for _, attr in run.kern.jac_items].index(None)]
        coeffs = stencil_coefficients(items, tuple(buf.shape[1:]), period=problem.domain.cshape)
        return value.clone(), coeffs.clone()

    return run_threads(world, body)


@pytest.mark.parametrize("double", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,sigma,shape,world", [(k, 0.0, s, w) for k in ("jump", "nonlinear") for s, w in CASES]
                         + [("smooth", 1.0, "cube", 4), ("smooth", 1.0, "box", 3)])
def test_slab_jacobian_matches_undivided(kind, sigma, shape, world, double):
    from odil_amd import gmg

    problem, state = make(kind, SHAPES[shape], double, sigma)
    vector, op = problem.linearize_device(state)
    ref = gmg.recognise_stencil(op)
    assert ref is not None
    ref_v = vector.view(SHAPES[shape])
    scale = float(ref.abs().max())
    bound = (1e-13 if double else 1e-5) * scale
    n = SHAPES[shape][0] // world
    worst = 0.0
    for rank, (value, coeffs) in enumerate(slab_jacobians(problem, state, world)):
        planes = slice(rank * n, (rank + 1) * n)
        dv = float((value - ref_v[planes]).abs().max())
        dc = (coeffs - ref[:, planes]).abs()
        assert torch.isfinite(coeffs).all() and torch.isfinite(value).all()
        assert dv <= bound and float(dc.max()) <= bound, (rank, dv, float(dc.max()), bound)
        worst = max(worst, dv, float(dc.max()))
    # the same expressions evaluated on the same values: bit-identical in float64 (float32 kernels may contract to FMA)
    assert worst == 0.0 or not double, "slab k_jac differs from the undivided one by {:.3e} (max |c| {:.3e})".format(worst, scale)


def newton_args(linsolver="multigrid", tol=1e-12, epochs=3):
    return argparse.Namespace(linsolver=linsolver, linsolver_tol=tol, linsolver_maxiter=None, linsolver_damp=0,
                              linsolver_dampdiag=0, linsolver_verbose=0, epochs=epochs, epoch_start=0)


def undivided_newton(problem, state, args):
    """util.optimize_newton: the iterates and the losses after every step."""
    from odil_amd.util import optimize_newton

    iterates, losses = [], []

    def callback(state, epoch, pinfo):
        if epoch > 0:
            iterates.append(state.fields["u"].array.clone())
            losses.append(float(pinfo["loss"]))

    optimize_newton(args, problem, state, callback=callback)
    return iterates, losses


def slab_newton(problem, state, world, args):
    from odil_amd.slab_solvers import SlabTracedNewton, run_threads
    from odil_amd.slab_traced import SlabTracedAdam

    def body(rank, comm):
        run = SlabTracedAdam(problem, state, rank, world, kernels=jac_kernels)
        newton = SlabTracedNewton(run, args.linsolver, args.linsolver_tol, args.linsolver_maxiter)
        steps = []
        for _ in range(args.epochs):
            status = dict(newton.step(comm))
            steps.append((run.owned_arrays()[0].clone(), run.last_loss(comm), status))
        return steps

    return run_threads(world, body)


@pytest.mark.parametrize("double", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,world", [("cube", 1), ("cube", 2), ("cube", 4), ("box", 2), ("box", 3), ("box", 4)])
@pytest.mark.parametrize("kind", ["jump", "nonlinear"])
def test_newton_steps_match_undivided(kind, shape, world, double):
    args = newton_args()
    # (48 x 32 x 16: the slab cycle contracts by about 0.7 per cycle there -- 7e-8 after 60 cycles for 'jump' -- and needs
    # about 100 cycles to 1e-12; the default cap of 60 would refuse the step)
    args.linsolver_maxiter = 200
    problem, state = make(kind, SHAPES[shape], double, random=False)
    ranks = slab_newton(problem, state, world, args)  # (the state itself is not changed by the slab runs)
    problem, state = make(kind, SHAPES[shape], double, random=False)
    iterates, losses = undivided_newton(problem, state, args)
    n = SHAPES[shape][0] // world
    loss0 = float(problem.eval_loss_grad_device(make(kind, SHAPES[shape], double, random=False)[1])[0])
    for k in range(args.epochs):
        want = iterates[k]
        scale = float(want.abs().max())
        for rank, steps in enumerate(ranks):
            u, loss, status = steps[k]
            # converged, or (the single-GPU rule) stopped at the rounding floor: 'jump' on 48 x 32 x 16 in float64 stops at
            # 2.5e-12 after 93 cycles
            assert status["converged"] or (status["stagnated"] and status["residual"] <= (1e-11 if double else 1e-3)), (
                k, rank, status)
            assert status == ranks[0][k][2], "ranks disagree on the solver status"
            err = float((u - want[rank * n:(rank + 1) * n]).abs().max())
            assert err <= (1e-8 if double else 1e-4) * scale, (k, rank, err, scale)
            assert abs(loss - losses[k]) <= loss_bound(losses[k], loss0, double), (k, loss, losses[k], loss0)


def loss_bound(ref, loss0, double=True):
    """1e-8 relative (1e-4 in float32), with a floor where a step has solved a (nearly) linear problem and the loss is
    that of the linear solver's residual and the rounding of the residual itself: the residual norms agree to 1e-10 (f64)
    / 1e-3 (f32) of the initial one."""
    return (1e-8 if double else 1e-4) * abs(ref) + (1e-20 if double else 1e-6) * loss0


@pytest.mark.parametrize("world", [2, 3, 4])
def test_newton_refuses_an_unconverged_step(world):
    """A solve cut off by `linsolver_maxiter` (2 cycles, far from 1e-12 and too few to count as stagnated): the step must
    raise, name the residual, and leave every rank's unknowns as they were -- never be applied."""
    from odil_amd.slab_solvers import SlabTracedNewton, ThreadComm
    from odil_amd.slab_traced import SlabTracedAdam
    import threading

    problem, state = make("jump", SHAPES["box"], random=False)
    shared = ThreadComm.Shared(world)
    seen = [None] * world

    def work(rank):
        with ThreadComm(rank, shared) as comm:
            run = SlabTracedAdam(problem, state, rank, world, kernels=jac_kernels)
            x0 = run.x.clone()
            try:
                SlabTracedNewton(run, "multigrid", 1e-12, maxiter=2).step(comm)
            except RuntimeError as e:
                seen[rank] = (str(e), torch.equal(run.x, x0))

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(s is not None and "relative residual" in s[0] and s[1] for s in seen), seen
    assert len({s[0] for s in seen}) == 1  # the same decision and the same residual on every rank


def test_newton_direct_matches_undivided():
    args = newton_args("direct", tol=1e-10, epochs=2)
    problem, state = make("nonlinear", SHAPES["cube"], random=False)
    ranks = slab_newton(problem, state, 2, args)
    problem, state = make("nonlinear", SHAPES["cube"], random=False)
    loss0 = float(problem.eval_loss_grad_device(state)[0])
    iterates, losses = undivided_newton(problem, state, args)
    for k in range(args.epochs):
        want = iterates[k]
        for rank, steps in enumerate(ranks):
            u, loss, status = steps[k]
            assert status["converged"] and status["residual"] <= 1e-12
            assert float((u - want[rank * 16:(rank + 1) * 16]).abs().max()) <= 1e-8 * float(want.abs().max())
            assert abs(loss - losses[k]) <= loss_bound(losses[k], loss0), (k, loss, losses[k])


# ---- refusals ----------------------------------------------------------------------------------------------------------
def refusal_case(name):
    import diffusion as ex

    args = newton_args(epochs=2)
    axis = None
    if name == "2-D":
        args = ex.parse_args(["--ndim", "2", "--N", "16", "--epochs", "2"])
        problem, state = ex.make_problem(args)
    elif name == "darcy":
        import darcy

        args = darcy.parse_args(["--ndim", "3", "--N", "8", "--epochs", "2", "--optimizer", "newton"])
        problem, state = darcy.make_problem(args)
    elif name == "multigrid field":
        args = ex.parse_args(["--ndim", "3", "--N", "16", "--epochs", "2", "--multigrid", "1"])
        problem, state = ex.make_problem(args)
    else:
        problem, state = make("periodic" if name == "periodic" else "jump", (16, 16, 16))
        if name == "axis 1":
            axis = 1
        elif name == "damping":
            args.linsolver_damp = 1e-3
        elif name == "cg":
            args.linsolver = "cg"
    args.optimizer = "newton"
    args.report_every = 1
    args.lr = 1e-3
    return args, problem, state, axis


@pytest.mark.parametrize("name", ["2-D", "axis 1", "darcy", "multigrid field", "damping", "cg", "periodic"])
def test_refusals_leave_the_state_unchanged(name):
    from odil_amd.slab_traced import optimize_slab

    args, problem, state, axis = refusal_case(name)
    before = [a.clone() for a in problem.domain.arrays_from_state(state)]
    with pytest.raises(NotImplementedError, match="slab decomposition"):
        optimize_slab(args, problem, state, axis=axis)
    after = problem.domain.arrays_from_state(state)
    assert all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("world", [2, 4])
def test_periodic_cut_axis_refused_on_every_rank_before_any_update(world):
    from odil_amd.slab_solvers import SlabTracedNewton, ThreadComm
    from odil_amd.slab_traced import SlabTracedAdam
    import threading

    problem, state = make("periodic", (16, 16, 16))
    shared = ThreadComm.Shared(world)
    seen = [None] * world

    def work(rank):
        with ThreadComm(rank, shared) as comm:
            run = SlabTracedAdam(problem, state, rank, world, kernels=jac_kernels)
            x0 = run.x.clone()
            try:
                SlabTracedNewton(run).step(comm)
            except NotImplementedError as e:
                seen[rank] = (str(e), torch.equal(run.x, x0))

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(s is not None and "periodic" in s[0] and s[1] for s in seen), seen


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_example_newton_slab_decomposed_under_torch_distributed(tmp_path):
    """examples/diffusion/diffusion.py --slab 1 --optimizer newton under torch.distributed.run (two ranks, gloo, this box's
    GPU) against the same example run undivided: the same losses after every step, the same final field."""
    import odil_amd as odil

    script = os.path.join(ROOT, "examples", "diffusion", "diffusion.py")
    common = ["--ndim", "3", "--N", "32", "--optimizer", "newton", "--epochs", "3", "--kind", "jump", "--linsolver_tol",
              "1e-12", "--plot_every", "100", "--checkpoint_every", "0", "--report_every", "1", "--history_every", "1"]
    env = dict(os.environ, ODIL_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    slab_dir, one_dir = str(tmp_path / "slab"), str(tmp_path / "one")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29500 + os.getpid() % 200), script, "--slab", "1", "--outdir", slab_dir] + common
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"ranks=2 loss=([0-9.eE+-]+)", open(os.path.join(slab_dir, "train.log")).read())]
    assert len(losses) == 3
    out = subprocess.run([sys.executable, script, "--outdir", one_dir, "--write_u", "1"] + common, env=env, capture_output=True, text=True,
                         timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    rows = open(os.path.join(one_dir, "train.csv")).read().split()
    keys = rows[0].split(",")
    ref = [float(r.split(",")[keys.index("loss")]) for r in rows[1:]][-3:]  # (after each of the three steps)
    # (the initial loss, for the floor of loss_bound: the residual norm the undivided run reports at epoch 0)
    loss0 = float(re.search(r"residual: [^:]*:([0-9.eE+-]+)", open(os.path.join(one_dir, "train.log")).read()).group(1)) ** 2
    # (train.log carries 8 significant digits)
    assert len(ref) == 3 and all(abs(a - b) <= loss_bound(b, loss0) + 1e-8 * abs(b) for a, b in zip(losses, ref)), (losses, ref)
    got, meta = odil.read_raw_with_xmf(os.path.join(slab_dir, "u_final.xmf"))
    want, _ = odil.read_raw_with_xmf(os.path.join(one_dir, "u_final.xmf"))
    assert got.shape == (32, 32, 32) and meta["name"] == "u"
    assert np.max(np.abs(got - want)) <= 1e-8 * np.max(np.abs(want))
