"""Drivers that run B problems side by side: `optimize_ensemble` (Adam) and `optimize_newton_ensemble` (Newton).  The
reference runs a sweep as B processes and has no counterpart; `util` re-exports both names next to `optimize_grad` /
`optimize_newton`, whose single runs every member reproduces.  Written once for both drivers: `_check_members`; for both
Newton routes: `_newton_loop`.  `printlog` and `_pinfo` are `util`'s (one log sink).
"""

import argparse

import numpy as np
import torch

from . import gmg, ops, util
from .core import Field
from .optimizer import make_optimizer

# what members are compared by -> how a refusal calls it
_LABELS = dict(shapes="level shapes", cshape="cells", dtype="dtype", device="device", spacing="grid spacing")


def _check_members(who, problems, states, describe):
    """The checks both drivers open with, structure only (no operator is probed, no state changes): as many states as
    problems, every state initialised with one unknown field, and `describe(b, problem, state, refuse) -> kind`, a dict
    of what the members must share (keys of `_LABELS`, compared in its order with member 0's) -- which also makes the
    driver's own refusals.  `refuse(member, reason)` raises ValueError("<who>: member <b>: <reason>").
    Returns (the kind all members share, refuse)."""
    if not problems or len(problems) != len(states):
        raise ValueError("{}: {} problems with {} states".format(who, len(problems), len(states)))

    def refuse(member, reason):
        raise ValueError("{}: member {}: {}".format(who, member, reason))

    first = None
    for b, (problem, state) in enumerate(zip(problems, states)):
        if not state.initialized:
            refuse(b, "uninitialized state, use `state = domain.init_state(state)`")
        if len(state.fields) != 1:
            refuse(b, "{} unknown fields (the Poisson problem has one)".format(len(state.fields)))
        kind = describe(b, problem, state, refuse)
        first = first or kind
        for what, value in kind.items():
            if value != first[what]:
                refuse(b, "{} {} differ from member 0's {}".format(_LABELS[what], value, first[what]))
    return first, refuse


def _evaluate(problem, state):
    """The pinfo of one member at its current state, as `optimize_grad` / `optimize_newton` report it."""
    loss, _, terms, names, norms = problem.eval_loss_grad_device(state)
    return util._pinfo(loss, terms, names, norms)


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
    if lrs is not None and len(lrs) != len(problems):
        raise ValueError("optimize_ensemble: {} step sizes for {} members".format(len(lrs), len(problems)))
    fused.ensemble_form(form, [(2,)], torch.float64)  # (any other value of `form` raises here)
    predicates = dict(workgroup=fused.small_refusal, launches=fused.launches_refusal, volumes=fused.volumes_refusal)

    def describe(b, problem, state, refuse):
        nonlocal form
        domain = problem.domain
        arrays = domain.arrays_from_state(state)
        shapes = [tuple(int(n) for n in a.shape) for a in arrays]
        if shapes[0] != tuple(domain.cshape):
            refuse(b, "the unknown is not a cell-centred field of the domain")
        if b == 0:
            form = fused.ensemble_form(form, shapes, arrays[0].dtype)
        reason = predicates[form](shapes, arrays[0].dtype)
        if reason is not None:
            refuse(b, reason)
        return dict(shapes=shapes, dtype=arrays[0].dtype, device=arrays[0].device,
                    spacing=[float(domain.step_by_dim(i)) for i in range(domain.ndim)])

    _, refuse = _check_members("optimize_ensemble", problems, states, describe)
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
    util.printlog("Running {} optimizer on an ensemble of {} members".format(opt.displayname, len(problems)))

    def callback_wrap(epoch, losses, norms):
        for b, state in enumerate(states):
            callback(b, state, epoch, util._pinfo(losses[b], [losses[b]], ensemble.names[b], [norms[b]]))

    if callback:
        callback_wrap.next_active = getattr(callback, "next_active", None)
        for b, (problem, state) in enumerate(zip(problems, states)):  # (the report of the start, as optimize_grad makes it)
            callback(b, state, args.epoch_start, _evaluate(problem, state))
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

    linsolver = getattr(args, "linsolver", "direct")
    if linsolver not in ("direct", "multigrid"):
        raise ValueError("optimize_newton_ensemble: linsolver '{}' (the one-workgroup Newton solves serve 'direct' and "
                         "'multigrid')".format(linsolver))
    if getattr(args, "linsolver_damp", 0) or getattr(args, "linsolver_dampdiag", 0):
        raise ValueError("optimize_newton_ensemble: damping (linsolver_damp / linsolver_dampdiag) is not served: the cycles "
                         "solve M d = r, which has the solution of the normal equations only without it")
    refused = dict(poisson=None, stencil=None)  # per route the first (member, reason) it refuses while the other admits

    def describe(b, problem, state, refuse):
        domain = problem.domain
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
        reasons = dict(poisson=fused.newton_refusal(cshape, [npdt(v) ** 2 for v in kind["spacing"]], dtype),
                       stencil=fused.newton_stencil_refusal(cshape, dtype))
        if None not in reasons.values():
            refuse(b, reasons["poisson"])
        for route, reason in reasons.items():
            if reason is not None and refused[route] is None:
                refused[route] = (b, reason)
        return kind

    kind, refuse = _check_members("optimize_newton_ensemble", problems, states, describe)
    evaluators = []
    for problem, state in zip(problems, states):
        problem.recognise(state)
        ev = getattr(problem, "_fused", None)
        evaluators.append(ev if ev is not None and ev.nlvl == 1 else None)
    route = "stencil" if any(ev is None for ev in evaluators) else "poisson"
    if refused[route] is not None:
        refuse(*refused[route])
    if route == "poisson":  # (one launch per epoch: the whole Newton step on the packed iterate and right-hand sides)
        ev = evaluators[0]
        solver = gmg.EnsembleGMG(ev.cshape, ev.h2, ev.dtype, ev.device, len(evaluators))
        rhs = torch.stack([e.rhs.reshape(ev.cshape) for e in evaluators])
        step = lambda u, first, tol, maxcycles: solver.newton_step(u, rhs, tol=tol, maxcycles=maxcycles)
    else:
        solver, step = _stencil_route(args, problems, states, kind)
    return _newton_loop(args, problems, states, callback, linsolver, kind["dtype"], route, solver, step)


def _stencil_route(args, problems, states, kind):
    """(solver, step) of the route for members that are not all the Poisson operator (the docstring of
    `optimize_newton_ensemble`); the members have passed its checks, `kind` is what they share.  Linearises once here,
    before any state changes: a member that has no stencil Jacobian is named first.  Without an epoch to run, no solver."""
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

    solver = None
    if args.epochs > args.epoch_start:
        linearise(stage)
        solver = gmg.EnsembleGMG.from_coeffs(stage)
    del stage

    def step(u, first, tol, maxcycles):
        if not first:
            linearise(solver.fine)
            solver.rebuild()
        solver.solve(r, d, tol=tol, maxcycles=maxcycles, start=2)  # M_b d_b = r_b, the convention of optimize_newton
        ops.axpy(u.view(-1), d.view(-1), -1.0)                     # u -= d for all members

    return solver, step


def _newton_loop(args, problems, states, callback, linsolver, dtype, route, solver, step):
    """What the Newton routes share.  route: "poisson" / "stencil"; solver: its gmg.EnsembleGMG (None only when no epoch
    runs); step(u, first, tol, maxcycles) advances the packed iterate u [B, *cshape] by one Newton step of every member
    (first: at args.epoch_start) and leaves solver.outcome / status(b) behind."""
    from . import linsolver as ls

    nb = len(problems)
    u = torch.stack([problem.domain.arrays_from_state(state)[0].to(dtype) for problem, state in zip(problems, states)])
    for b, (problem, state) in enumerate(zip(problems, states)):
        problem.domain.arrays_to_state([u[b]], state)  # (views of the packed iterate: always the current one)
    tol, maxcycles = ls.cycle_budget(linsolver, getattr(args, "linsolver_tol", 1e-10), getattr(args, "linsolver_maxiter", None))
    tol = max(tol, 50 * float(torch.finfo(dtype).eps))
    util.printlog("Running Newton optimizer on an ensemble of {} members{}".format(
        nb, " (variable-coefficient stencils)" if route == "stencil" else ""))

    def report(epoch, stepped):
        for b, (problem, state) in enumerate(zip(problems, states)):
            pinfo = _evaluate(problem, state)
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
        step(u, epoch == args.epoch_start, tol, maxcycles)
        k = epoch - args.epoch_start
        cycles[:, k] = solver.outcome[:, 0]
        residuals[:, k] = [solver.status(b)["residual"] for b in range(nb)]
        if getattr(args, "linsolver_verbose", 0):
            util.printlog([solver.status(b) for b in range(nb)])
        if callback and epoch + 1 >= due:
            report(epoch + 1, True)
            due = next_active(epoch + 1) if next_active else epoch + 2
    arrays = [problem.domain.arrays_from_state(state) for problem, state in zip(problems, states)]
    return arrays, argparse.Namespace(epochs=args.epochs, evals=nepochs, cycles=cycles, residuals=residuals, solver=solver,
                                      route=route)
