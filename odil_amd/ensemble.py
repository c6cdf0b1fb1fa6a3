"""Drivers that run B problems side by side: `optimize_ensemble` (Adam, L-BFGS-B) and `optimize_newton_ensemble` (Newton).  The
reference runs a sweep as B processes and has no counterpart; `util` re-exports both names next to `optimize_grad` /
`optimize_newton`, whose single runs every member reproduces.  Written once for both drivers: `_check_members`; for both
Newton routes: `_newton_loop`.  `linearize_ensemble` (`EnsembleLinearizer`) is the linearisation of the Newton driver's
stencil route, all members in one generated launch; the Adam driver's route for members that are not all the Poisson
stencil is `fused.TracedLaunchEnsemble` (any number of grid unknowns at one location of 'c' / 'n').  `printlog` and `_pinfo` are `util`'s (one log sink).
"""

import argparse
import math
import os

import numpy as np
import torch

from . import gmg, ops, util
from .core import Array, Field, NeuralNet, Problem
from .optimizer import make_optimizer

# what members are compared by -> how a refusal calls it
_LABELS = dict(shapes="level shapes", cshape="cells", dtype="dtype", device="device", spacing="grid spacing",
               fields="grid unknowns (key, position in the state)", loc="location",
               params="Array unknowns (key, position in the state, shape)",
               nets="NeuralNet unknowns (key, position in the state, layer shapes)")


def _check_members(who, problems, states, describe, arrays_ok=False):
    """The checks both drivers open with, structure only (no operator is probed, no state changes): as many states as
    problems, every state initialised with one unknown field (arrays_ok: `Array` unknowns beside it do not count, nor do
    `NeuralNet` unknowns beside a grid field under a key where member 0 has a network beside its grid field; and the
    members may have SEVERAL unknown fields, every member as many as member 0 -- what they are is `describe`'s), and
    `describe(b, problem, state, refuse) -> kind`, a dict of what the members must share (keys of `_LABELS`, compared in
    its order with member 0's) -- which also makes the driver's own refusals.  `refuse(member, reason)` raises
    ValueError("<who>: member <b>: <reason>").
    Returns (the kind all members share, refuse)."""
    if not problems or len(problems) != len(states):
        raise ValueError("{}: {} problems with {} states".format(who, len(problems), len(states)))

    def refuse(member, reason):
        raise ValueError("{}: member {}: {}".format(who, member, reason))

    first, net_keys, nfirst = None, set(), 1
    for b, (problem, state) in enumerate(zip(problems, states)):
        if not state.initialized:
            refuse(b, "uninitialized state, use `state = domain.init_state(state)`")
        nfields = sum(1 for f in state.fields.values() if not (arrays_ok and isinstance(f, Array)))
        if arrays_ok:
            nets = [key for key, f in state.fields.items() if isinstance(f, NeuralNet)]
            if len(nets) < nfields:  # (the state also holds a grid field)
                if b == 0:
                    net_keys = set(nets)
                nfields -= sum(1 for key in nets if key in net_keys)
        if arrays_ok and b == 0 and nfields > 1:
            nfirst = nfields
        if nfields != nfirst:
            refuse(b, "{} unknown fields ({})".format(nfields, "the Poisson problem has one" if nfirst == 1 else
                                                      "member 0 has {}".format(nfirst)))
        kind = describe(b, problem, state, refuse)
        first = first or kind
        for what, value in kind.items():
            if value != first[what]:
                refuse(b, "{} {} differ from member 0's {}".format(_LABELS[what], value, first[what]))
    return first, refuse


def _plain_field(b, problem, state, refuse):
    """What the Newton routes compare of member b, whose unknown must be ONE plain cell-centred `Field` of the domain."""
    domain = problem.domain
    (field,) = state.fields.values()
    if type(field) is not Field:
        refuse(b, "the unknown is a {} (a plain Field is needed: no multigrid decomposition)".format(type(field).__name__))
    cshape = tuple(int(n) for n in domain.cshape)
    if tuple(int(n) for n in field.array.shape) != cshape or field.loc != "c" * domain.ndim:
        refuse(b, "the unknown is not a cell-centred field of the domain")
    return dict(cshape=cshape, dtype=field.array.dtype, device=field.array.device,
                spacing=[float(domain.step_by_dim(i)) for i in range(domain.ndim)])


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

    args.optimizer must be 'adam' / 'adamn' (or 'lbfgsb': the last paragraph); lrs: one step size per member (default
    args.lr for all).
    callback(member, state, epoch, pinfo): called for every member at args.epoch_start (the initial evaluation) and at
    the epochs its `next_active(epoch)` attribute names (the cadence of `make_callback`; without the attribute: every
    epoch), pinfo as `optimize_grad` reports it, device scalars read lazily.  The callback reads the state; arrays it
    swaps in are not picked up.
    Members must be the recognised Poisson operator, share cshape, level shapes, spacing, dtype and device, and be
    admitted by the form that runs them (fused.small_refusal: small enough for the one-workgroup epochs;
    fused.launches_refusal: 1-D / 2-D, at least two levels that halve; fused.volumes_refusal: 3-D, at least two levels
    that halve, a finest extent of at least 4); anything else raises ValueError naming the first
    offending member -- structure (shapes, size) is checked for all members before any operator is probed.

    When not every member is that Poisson operator and form is 'launches', 'volumes' or 'auto' (with operators traced,
    `runtime.enable_trace`, and members on a device), ALL members run as the traced stencil operators they are
    (optinfo.route == "traced", fused.TracedLaunchEnsemble): every epoch is the launches of a single traced run -- the
    synthesis, the generated forward kernels and gathers (`stencil_bind.EpochBatch`: one launch per group of members whose
    operators generate the same source), the transposed prolongations with the updates of the coarser levels, and
    `ops.adam_step_batch` for level 0 -- each covering all members.  'auto' then picks by dimension ('volumes' for 3-D and 4-D).
    Such members have ANY NUMBER of grid unknowns (and possibly `Array` unknowns: next paragraph), each a plain `Field` (one
    level: no transfers, exempt from the two-level rule of the forms) or a `MultigridField` with all factors 1 that coarsens
    every axis, on a 1-D to 4-D grid (4-D: velocity_from_tracer/veltracer3d, u, vx, vy, vz at 'nccc' on (t, x, y, z); form
    'volumes' reads as "three dimensions and more", 'launches' refuses them by name).  The grid unknowns of a member share ONE location string, any mix of 'c' and 'n'
    (velocity_from_tracer: u, vx, vy at 'ncc'; heat_tmax and infer_constant: a field at 'nc' beside an `Array`), one kind
    and the same level shapes -- an operator whose fields or outputs live on several grids stays refused -- and all members
    share keys, positions in the state, location and level shapes (else ValueError naming the member, before any state
    changes and before any operator is traced).  The F fields of the B members are stacked on the member axis: one
    [F B, *shape] tensor per level, row f B + b, so the synthesis, the transposed chain with the updates of the coarser
    levels (`ops.mg_synth_adj_adam_members`) and the level-0 update are each ONE set of launches for all fields of all
    members; ONE cell-centred unknown makes exactly the launches it always made.  The level shapes must be admitted by
    `fused.traced_refusal` (members whose finest array is no multiple of 16 bytes are refused -- every float64 1-D
    node-centred field among them --, and the library says whether every level of the stacked rows computes what that
    level of one member computes: odil_mg_members_levels_ok); operators whose kernels have no batched form (marching
    kernels, outputs in parameter space that only the torch replay evaluates) raise ValueError naming the member.  The callback's pinfo carries the member's own
    names, terms and norms.  Epochs are replayed as a graph only when no member has host scalars (functions of
    `problem.tracers`), which travel in the argument blocks and are uploaded again when they change.  With
    form='workgroup', or without tracing, a member that is not the Poisson operator stays refused.

    INVERSE PROBLEMS run on that traced route: beside its one grid unknown a member may have any number of `Array`
    unknowns (constants that the grid residuals multiply stencil terms by: `ctx.field(key)[k]`), of any shape, anywhere in
    the state -- the same keys, shapes and positions for all members (else ValueError naming the member, before any state
    changes).  The members' constants live in packed [B, P] tensors beside the level arrays; every member's kernels read
    its own row and reduce the gradient of its constants over the grid as its single run does, and ONE launch per epoch
    (`ops.adam_step_params_batch`) updates the constants of all members.  The arrays returned for member b, and those its
    state holds afterwards, are all its arrays in `arrays_from_state` order, the `Array`s included, and every one ends where
    the member's own `optimize_grad` run ends, bit for bit, with Adam and with L-BFGS-B (whose member-major vectors hold the
    constants where the single run's packed vector has them).
    `NeuralNet` unknowns (pointwise networks the residuals evaluate: the conductivity `sigmoid(MLP(u)) kmax` of
    examples/heat) stand beside the field like the `Array`s: the same keys, positions and layer shapes for all members,
    the same dtype and device as the field (else ValueError naming the member, before any state changes and before any
    operator is traced); their weights and biases live in the same packed [B, P] tensors, weights then biases as
    `arrays_from_state` has them.  Outputs in PARAMETER space -- heat's `wreg`, a weight decay, a prior on an `Array` -- are
    evaluated by one generated launch per epoch (`k_par_batch`), their terms and norms reported at their outputs'
    positions under the member's names.
    Host scalars: regularisers annealed with the epoch read `ctx.tracers["epoch"]`.  The callback is where to advance
    `problems[member].tracers["epoch"]`, exactly as the callback of a single run does (`make_callback`); such members are
    not replayed as a graph, and their argument blocks are uploaded again when a value has changed.
    Not served: marching kernels (float32 members of three or more dimensions with a last axis of at least 128 cells),
    parameter-space outputs that only the torch replay evaluates (reductions, broadcasts: `param_expr.Unsupported`), Newton
    -- ValueError naming the member -- and, because a single run packs its arrays back to back and its 3-D transfer
    kernels choose by alignment, a number of elements (`Array`, `NeuralNet`, earlier grid fields) before a 3-D or 4-D
    multigrid field that is no multiple of 4 (put the parameters after the fields).  `optimize_newton_ensemble` keeps refusing members with `Array` or
    `NeuralNet` unknowns.
    Returns ([arrays of member b: its level arrays; with `Array` / `NeuralNet` unknowns all its arrays in state order], optinfo);
    optinfo.losses / .norms: [B, epochs] device tensors; optinfo.route: "poisson" or "traced"; optinfo.form: the form that
    ran.

    args.optimizer == 'lbfgsb' runs L-BFGS-B on all members in LOCK-STEP (`LbfgsbOptimizer.run_ensemble`), on both routes,
    with form 'launches', 'volumes' or 'auto' ('auto' by dimension; 'workgroup', the default, raises ValueError: the
    whole-epoch kernels are Adam; so does `lrs`).  Route selection and structural checks are those above.  A round is ONE
    evaluation of all members (the launches of an epoch without any update: `BatchedLaunches.loss_grad`), the batched
    vector algebra (`ops.lbfgs_*_batch`, each launch over the list of members that need it) and two host reads -- the cost
    of one iteration of a single run, whatever B is.  Members progress independently: one in the middle of a line search
    evaluates again while others accept their step; a member retires when it has made args.epochs iterations, converges
    (args.bfgs_pgtol) or its line search fails with an empty memory, and is evaluated along but never touched.  Every
    member ends where its own `optimize_grad(args, "lbfgsb", problem, state)` run ends, bit for bit.  args.bfgs_m (at most
    64: ValueError beyond), bfgs_maxls and bfgs_pgtol as in `optimize_grad`; the history of all members takes
    B 2 m n 8 bytes, refused (ValueError naming the bytes) before any state changes when the device has less free.
    No EarlyStopError: optinfo.tasks / .warnflags / .nits / .evals ([B]) say how each member ended; optinfo.rounds,
    .host_reads, .read_seconds (host time blocked in the reads), .ensemble.  The callback is called for member b at the
    start and after those of ITS OWN iterations that `next_active` names, when its state shows the iterate it has just
    accepted; at return every state holds its member's last accepted iterate.  Eager: no graph replay."""
    from . import fused, runtime

    optname = getattr(args, "optimizer", "adam")
    if optname not in ("adam", "adamn", "lbfgsb"):
        raise ValueError("optimize_ensemble runs Adam ('adam' / 'adamn') and L-BFGS-B ('lbfgsb'), not optimizer '{}'".format(optname))
    lbfgsb = optname == "lbfgsb"
    if lbfgsb:
        if form == "workgroup":
            raise ValueError("optimize_ensemble: form 'workgroup' runs whole Adam epochs in one launch; optimizer 'lbfgsb' runs "
                             "as batched launches: form='launches', 'volumes' or 'auto'")
        if lrs is not None:
            raise ValueError("optimize_ensemble: step sizes `lrs` are Adam's; the line search of L-BFGS-B finds its own")
        for src, dst in [("bfgs_m", "m"), ("bfgs_pgtol", "pgtol"), ("bfgs_maxls", "maxls")]:  # (as optimize_grad)
            if getattr(args, src, None) is not None:
                kwargs[dst] = getattr(args, src)
        opt = make_optimizer(optname, dtype=problems[0].domain.dtype if problems else None, **kwargs)
        if opt.m > opt.max_ensemble_m:
            raise ValueError("optimize_ensemble: " + opt.ensemble_refusal(len(problems), 0, "cpu"))
    if lrs is not None and len(lrs) != len(problems):
        raise ValueError("optimize_ensemble: {} step sizes for {} members".format(len(lrs), len(problems)))
    fused.ensemble_form(form, [(2,)], torch.float64)  # (any other value of `form` raises here)
    predicates = dict(workgroup=fused.small_refusal, launches=fused.launches_refusal, volumes=fused.volumes_refusal)
    # members that are not all the Poisson stencil run as traced operators (fused.TracedLaunchEnsemble) where the caller
    # asked for batched launches and operators are traced at all; which route runs is known once the operators are probed
    # (the generated kernels need a device: members on CPU tensors keep the refusals of the Poisson forms, as before)
    requested, traceable = form, form != "workgroup" and runtime.enable_trace and torch.cuda.is_available()
    late = dict(poisson=None, traced=None)  # per route the first (member, reason) it refuses while the other admits
    unserved = []  # (member, reason) of members with `Array` unknowns when no traced route runs at all

    def describe(b, problem, state, refuse):
        nonlocal form, traceable
        domain = problem.domain
        # the grid unknowns (their level arrays) and the `Array` unknowns beside them, by position in `arrays_from_state`
        # (and the `NeuralNet` unknowns, when the state holds a grid field at all: a network alone is "the unknown")
        params, nets, grids = [], [], []
        beside = any(not isinstance(field, (Array, NeuralNet)) for field in state.fields.values())
        for pos, (key, field) in enumerate(state.fields.items()):
            if isinstance(field, Array):
                params.append((key, pos, tuple(int(n) for n in field.array.shape)))
            elif beside and isinstance(field, NeuralNet):
                nets.append((key, pos, [tuple(int(n) for n in a.shape) for a in domain.arrays_from_field(field)]))
            else:
                grids.append((key, pos, field, domain.arrays_from_field(field)))
        key0, upos, unknown, arrays = grids[0]
        shapes = [tuple(int(n) for n in a.shape) for a in arrays]
        loc = getattr(unknown, "loc", None)
        if not isinstance(loc, str) or len(loc) != domain.ndim or any(c not in "cn" for c in loc):
            refuse(b, "the unknown is not a cell-centred field of the domain")
        if shapes[0] != tuple(domain.size(loc=loc)):
            refuse(b, "the unknown is not a cell-centred field of the domain" if loc == "c" * domain.ndim else
                   "the unknown '{}' at '{}' has the shape {}, a field of the domain has {}".format(
                       key0, loc, shapes[0], tuple(domain.size(loc=loc))))
        for key, _, field, held in grids[1:]:  # (several grid unknowns: one grid, one kind, one location)
            if type(field) is not type(unknown):
                refuse(b, "grid unknowns of two kinds: '{}' is a {}, '{}' a {}".format(key0, type(unknown).__name__, key,
                                                                                      type(field).__name__))
            if getattr(field, "loc", None) != loc:
                refuse(b, "grid unknowns at two locations: '{}' at '{}', '{}' at '{}' (operators whose fields live on "
                          "several grids are not served)".format(key0, loc, key, getattr(field, "loc", None)))
            other = [tuple(int(n) for n in a.shape) for a in held]
            if other != shapes:
                refuse(b, "grid unknowns with different level shapes: '{}' {}, '{}' {}".format(key0, shapes, key, other))
            if held[0].dtype != arrays[0].dtype or held[0].device != arrays[0].device:
                refuse(b, "grid unknown '{}' is a {} tensor on {} ('{}': {} on {})".format(
                    key, held[0].dtype, held[0].device, key0, arrays[0].dtype, arrays[0].device))
        # anything but ONE cell-centred unknown is served by the traced route alone, like `Array` and `NeuralNet` unknowns
        many = len(grids) > 1 or loc != "c" * domain.ndim
        if b == 0:
            # (L-BFGS-B has no one-workgroup form: 'auto' picks among the batched launches, by dimension)
            form = _traced_form(form, shapes) if lbfgsb or many else fused.ensemble_form(form, shapes, arrays[0].dtype)
            traceable = traceable and arrays[0].is_cuda
        reasons = dict(poisson=predicates[form](shapes, arrays[0].dtype) if not many else None, traced=None)
        if params or nets or many:  # (inverse problems: the traced route alone serves them)
            count = " and ".join("{} {} unknown{}".format(len(lst), name, "" if len(lst) == 1 else "s")
                                 for lst, name in ((params, "Array"), (nets, "NeuralNet")) if lst)
            what = "{} beside the field".format(count) if count else (
                "{} grid unknowns".format(len(grids)) if len(grids) > 1 else "a grid unknown at '{}'".format(loc))
            if count and many:
                what += ", {}".format("{} grid unknowns".format(len(grids)) if len(grids) > 1 else "the field at '{}'".format(loc))
            reasons["poisson"] = ("{}: such members run as traced operators -- form='launches', "
                                  "'volumes' or 'auto', with operators traced and the members on a device".format(what))
            if domain.ndim == 4:  # (said first: how the traced route lays 4-D members out, and what that needs)
                reasons["poisson"] = ("4-D grid: the batched launches of traced operators run 1-D to 3-D grids as a leading "
                                      "axis of the level arrays and 4-D grids as stacked rows on a grid dimension (form="
                                      "'volumes' or 'auto'); " + reasons["poisson"])
        if traceable or many:  # (what is not one cell-centred unknown: its structure is checked wherever it runs)
            reasons["traced"] = _traced_member(domain, [g[2] for g in grids], shapes, arrays[0].dtype,
                                               _traced_form(requested, shapes), loc)
            for _, gpos, _, _ in grids:  # (elements in front of every grid field: parameters and earlier grid fields)
                ahead = sum(math.prod(shape) for _, pos, shape in params if pos < gpos)
                nets_ahead = sum(math.prod(shape) for _, pos, shapes_ in nets if pos < gpos for shape in shapes_)
                ahead += nets_ahead + sum(a.numel() for _, pos, _, arrs in grids if pos < gpos for a in arrs)
                if reasons["traced"] is None and len(shapes[0]) >= 3 and len(shapes) > 1 and ahead % 4:
                    # a single run packs its arrays back to back: with `ahead` elements in front, the levels of its field are
                    # not aligned to four elements, and its 3-D transfers take other kernels (other rounding) than those of
                    # the members' aligned level arrays here.  4-D fields too: an 'nccc' level off the grid of two elements
                    # runs the fast transpose where the members' rows run the marching one.  Two elements would do for
                    # the 4-D transposes; the rule stays at 4 for 3-D and 4-D alike (one rule, and the prolongation of a
                    # single run picks its columns per thread by 16 bytes)
                    reasons["traced"] = ("{} {} elements stand before the {}-D multigrid field: a single run's level arrays are "
                                         "then not aligned to 4 elements and its transfer kernels round differently (put the "
                                         "{} after the field, or a multiple of 4 elements before it)".format(
                                             ahead, "Array and NeuralNet" if nets_ahead else "Array", len(shapes[0]),
                                             "NeuralNet" if nets_ahead else "Array"))
            held = [("Array", key, state.fields[key].array) for key, _, _ in params]
            held += [("NeuralNet", key, a) for key, _, _ in nets for a in domain.arrays_from_field(state.fields[key])]
            for what, key, array in held:
                if reasons["traced"] is None and (array.dtype != arrays[0].dtype or array.device != arrays[0].device):
                    reasons["traced"] = "{} unknown '{}' is a {} tensor on {} (the field: {} on {})".format(
                        what, key, array.dtype, array.device, arrays[0].dtype, arrays[0].device)
        if many and reasons["traced"] is not None:  # (structure: said wherever the members live)
            refuse(b, reasons["traced"])
        if (params or nets or many) and not traceable:  # (said once the members have been compared with each other: `unserved`)
            unserved.append((b, reasons["poisson"]))
        elif (params or nets) and reasons["traced"] is not None:  # (the only route that serves them says why it does not)
            refuse(b, reasons["traced"])
        elif reasons["poisson"] is not None and (not traceable or reasons["traced"] is not None):
            refuse(b, reasons["poisson"])
        for route, reason in reasons.items():
            if reason is not None and late[route] is None:
                late[route] = (b, reason)
        return dict(shapes=shapes, params=params, nets=nets, fields=[(key, pos) for key, pos, _, _ in grids], loc=loc,
                    dtype=arrays[0].dtype, device=arrays[0].device,
                    spacing=[float(domain.step_by_dim(i)) for i in range(domain.ndim)])

    kind, refuse = _check_members("optimize_ensemble", problems, states, describe, arrays_ok=True)
    if unserved:
        refuse(*unserved[0])
    evaluators = []
    for b, (problem, state) in enumerate(zip(problems, states)):
        problem.recognise(state)
        if getattr(problem, "_fused", None) is None:
            if traceable:
                break
            refuse(b, "the operator is not the recognised Poisson stencil ({})".format(
                "operators are not traced: ODIL_TRACE=0" if not runtime.enable_trace else
                "form='launches', 'volumes' or 'auto' run other stencil operators as traced kernels" if requested == "workgroup"
                else "the traced kernels of other stencil operators need members on a device"))
        evaluators.append(problem._fused)
    route = "poisson" if len(evaluators) == len(problems) else "traced"
    if late[route] is not None:
        refuse(*late[route])
    if route == "poisson":
        kind = dict(workgroup=fused.PoissonEnsemble, launches=fused.PoissonLaunchEnsemble, volumes=fused.PoissonVolumeEnsemble)[form]
        reason = kind.refusal(evaluators)
        if reason is not None:
            refuse(*reason)
        ensemble = kind(evaluators)
    else:  # (ALL members, the Poisson ones as the traced operators they are)
        form = _traced_form(requested, kind["shapes"])
        ensemble = _held_traced_ensemble(problems, states, kind, form)
    if lbfgsb:  # (before any state changes: the history of all members must fit the device)
        reason = opt.ensemble_refusal(ensemble.nbatch, ensemble.total, ensemble.device)
        if reason is not None:
            raise ValueError("optimize_ensemble: " + reason)
    for b, (problem, state) in enumerate(zip(problems, states)):
        levels = ensemble.levels(ensemble.x, b)
        for dst, src in zip(levels, problem.domain.arrays_from_state(state)):
            dst.copy_(src)
        problem.domain.arrays_to_state(levels, state)  # (views of the packed state: always the current iterate)

    if lbfgsb:
        return _lbfgsb_run(args, opt, problems, states, callback, ensemble, route, form)
    for src, dst in [("adam_epsilon", "epsilon"), ("adam_beta_1", "beta_1"), ("adam_beta_2", "beta_2")]:
        if getattr(args, src, None) is not None:
            kwargs[dst] = getattr(args, src)
    opt = make_optimizer(optname, dtype=problems[0].domain.dtype, mod=problems[0].domain.mod)
    util.printlog("Running {} optimizer on an ensemble of {} members".format(opt.displayname, len(problems)))

    def callback_wrap(epoch, losses, norms):
        if route == "traced":  # (the member's own names, terms and norms, as its `optimize_grad` run reports them)
            outs = [out.clone() for out in ensemble.outs]
            pouts = [None if pout is None else pout.clone() for pout in ensemble.pouts]
            for b, state in enumerate(states):
                loss, terms, member_norms = ensemble.report(b, outs, pouts)
                callback(b, state, epoch, util._pinfo(loss, terms, ensemble.names[b], member_norms))
            return
        for b, state in enumerate(states):
            callback(b, state, epoch, util._pinfo(losses[b], [losses[b]], ensemble.names[b], [norms[b]]))

    if callback:
        callback_wrap.next_active = getattr(callback, "next_active", None)
        for b, (problem, state) in enumerate(zip(problems, states)):  # (the report of the start, as optimize_grad makes it)
            callback(b, state, args.epoch_start, _evaluate(problem, state))
    arrays, optinfo = opt.run_ensemble(ensemble, epochs=args.epochs - args.epoch_start,
                                       callback=callback_wrap if callback else None, lr=args.lr, lrs=lrs,
                                       epoch_start=args.epoch_start, **kwargs)
    optinfo.route, optinfo.form = route, form
    return arrays, optinfo


def _lbfgsb_run(args, opt, problems, states, callback, ensemble, route, form):
    """The L-BFGS-B end of `optimize_ensemble`: the members are checked, `ensemble` holds their state (the states' arrays
    are views of it).  All members advance in lock-step (`LbfgsbOptimizer.run_ensemble`); the callback's pinfo is the
    member's last evaluation -- the one at the iterate it has just accepted -- copied before a later round overwrites it."""
    util.printlog("Running {} optimizer on an ensemble of {} members".format(opt.displayname, len(problems)))

    def report(b, epoch):
        if route == "traced":  # (the member's own names, terms and norms)
            k, j = ensemble.where[b]
            pout = ensemble.pouts[k]
            loss, terms, norms = ensemble.report(b, {k: {j: ensemble.outs[k][j].clone()}},
                                                 None if pout is None else {k: {j: pout[j].clone()}})
            callback(b, states[b], epoch, util._pinfo(loss, terms, ensemble.names[b], norms))
        else:
            loss = ensemble.loss[b].clone()
            callback(b, states[b], epoch, util._pinfo(loss, [loss], ensemble.names[b], [torch.sqrt(loss)]))

    if callback:
        report.next_active = getattr(callback, "next_active", None)
        for b, (problem, state) in enumerate(zip(problems, states)):  # (the report of the start, as optimize_grad makes it)
            callback(b, state, args.epoch_start, _evaluate(problem, state))
    arrays, optinfo = opt.run_ensemble(ensemble, epochs=args.epochs - args.epoch_start, callback=report if callback else None,
                                       epoch_start=args.epoch_start)
    optinfo.route, optinfo.form = route, form
    return arrays, optinfo


def _held_traced_ensemble(problems, states, kind, form):
    """The `fused.TracedLaunchEnsemble` of these (checked) members: the one kept on problems[0] when it was made for the
    same problem objects, kind and form and its traced operators still match the states (a sweep run again pays no second
    tracing of B operators), else a new one."""
    from . import fused

    held = getattr(problems[0], "_traced_ensemble", None)
    if not (held is not None and held[0] == (kind, form) and len(held[1]) == len(problems)
            and all(p is q for p, q in zip(held[1], problems))
            and all(t.matches(state) for t, state in zip(held[2].traced, states))):
        held = problems[0]._traced_ensemble = ((kind, form), list(problems), fused.TracedLaunchEnsemble(problems, states, form))
    return held[2]


def _traced_form(requested, shapes):
    """The form the traced route of `optimize_ensemble` runs members of these level shapes in: what the caller asked for,
    'auto' by dimension."""
    if requested == "auto":
        return "volumes" if len(shapes[0]) >= 3 else "launches"
    return requested


def _traced_member(domain, fields, shapes, dtype, form, loc):
    """Why a member whose grid unknowns are `fields` (all at `loc`, all of these level shapes) is not run by
    `fused.TracedLaunchEnsemble` in `form`, or None -- structure only: plain `Field`s or `MultigridField`s with all factors
    1 that coarsen every axis, level shapes that `fused.traced_refusal` admits.  (What stands beside them: the caller's.)"""
    from . import fused
    from .core import MultigridField

    for field in fields:
        if isinstance(field, MultigridField):
            factors = field.factors or domain.mg_factors or [1] * len(field.terms)
            if any(float(f) != 1.0 for f in factors):
                return "multigrid factors {} (the batched transfers run factors 1)".format([float(f) for f in factors])
            axes = field.axes or domain.mg_axes
            if axes is not None and not all(axes):
                return "multigrid axes {} (the batched transfers coarsen every axis)".format(list(axes))
            if len(shapes) < 2:  # (only a plain Field is the one-level case)
                return fused._too_few_levels(shapes)
        elif type(field) is not Field:
            return "the unknown is a {} (a Field or MultigridField is needed)".format(type(field).__name__)
    return fused.traced_refusal(shapes, dtype, form, loc=loc, nfields=len(fields))


def optimize_newton_ensemble(args, problems, states, callback=None, linearize="batched", time_linearize=False,
                             form="workgroup", krylov="never"):
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
    `fused.newton_stencil_refusal`, same cshape, spacing, dtype and device.  Per epoch: all members are linearised by ONE
    launch of the generated Jacobian kernel per group of members whose operators generate the same source
    (`linearize_ensemble`: `k_jac_batch` writes f(u) and the coefficient arrays straight into packed buffers allocated once;
    a member without a generated Jacobian, or whose reads share a stencil point, is linearised on its own), the hierarchies
    of all members are set up again in launches that do not grow with B (`gmg.EnsembleGMG.rebuild`: two per level, one for
    the dense coarsest matrices; the pseudo-inverses on the host), ONE launch solves M_b d_b = f_b(u_b) for all members and
    one forms u -= d.  A member whose Jacobian is no such stencil raises ValueError naming it at the first epoch, before any
    member is updated; so do members whose hierarchies do not coarsen along the same axes.  There is no fallback to the
    NORMAL EQUATIONS when a member's cycles do not contract (`optimize_newton` has one); with krylov='auto' a slow member is
    handed to GCR inside the launch (below), with krylov='never' its status reports converged=False or stagnated, and the
    caller decides.

    krylov: 'never' (the default), 'auto' or 'any'.  'auto', on both routes: a member whose cycles contract by less than
    0.5 well above the tolerance (the rule of `gmg.PoissonGMG.solve`) goes on with GCR(6) around the same cycle inside the solve launch
    (`gmg.EnsembleGMG(krylov="auto")`, odil_stencil_solve_krylov_batch) -- still one launch and one read-back per step;
    members that never meet the rule get the bits of 'never'.  Its work memory, B (2 m + 2) cells values more, must fit the
    free device memory: else ValueError naming the bytes, before any state changes.  optinfo.handover: [B, epochs], the
    cycle before which the member was handed over in that step, -1 where it was not; the member's status names it and
    reports method "... + GCR(6)".  Only form 'workgroup' serves 'auto': with form='launches', and with form='auto' when
    the members need the batched launches, ValueError (naming the member and the reason).
    krylov 'any': hand slow members over in whichever form runs them.  Where the one-workgroup form runs them it is 'auto'
    in everything (the same launch, bits and status).  Where the batched launches run them (form='launches', or
    form='auto' with members that need them) the solver is `gmg.EnsembleLaunchKrylovGMG`: the same decision order, pass
    algebra and stop reasons in one lock-step loop of passes across the launches, every decision on the device, four ints
    read back per pass; a handed-over member reports method "gmg-vcycle (variable coefficients), batched launches +
    GCR(6)", members that never meet the rule keep the bits of 'never'.  The same work memory is checked the same way.
    Any other value raises ValueError before any member is looked at.

    linearize (stencil route): "batched" is the above; "members" linearises member by member (`linearize_device`,
    `gmg.recognise_stencil`, copies into the packed buffers: B launches of `k_jac`) -- the same iterates, cycle counts and
    statuses bit for bit, kept as the reference of the tests and of timings.  time_linearize: device events around every
    linearisation, read after the last epoch (optinfo.linearize_ms).
    Returns ([arrays of member b], optinfo); optinfo.cycles / .residuals: [B, epochs] cycles run and final residual norms;
    optinfo.route: "poisson" or "stencil"; optinfo.linearize_launches: [epochs] Jacobian launches made per step (zeros on
    the Poisson route, which has no linearisation); optinfo.linearize_ms: [epochs] device time of the linearisations, None
    unless time_linearize; optinfo.form: the form that ran.

    form: 'workgroup' (the default) is all of the above, its refusals included: every member fits ONE workgroup
    (`gmg.EnsembleGMG.max_cells` cells: 32^3, 128^2).  'launches' runs members of any size that
    `fused.newton_launches_refusal` admits (256^2, 64^3, 128^3, ...): ALL members take the stencil route
    (optinfo.route == "stencil") with `gmg.EnsembleLaunchGMG` -- Poisson members included, whose Jacobian is a (2 d + 1)-point
    stencil like any other -- where every phase of the cycle on the levels too large for one workgroup is one launch that
    covers all members, the levels below are walked by one workgroup per member, and the convergence decision of every
    member stays on the device (one int per cycle read back for the whole ensemble).  `solver.method` is "gmg-vcycle
    (variable coefficients), batched launches".  Still no fallback to the normal equations, and damping stays refused.
    'auto': 'workgroup' where its checks admit the members, 'launches' otherwise.  Any other value raises ValueError before
    any member is looked at."""
    from . import fused

    if form not in ("workgroup", "launches", "auto"):
        raise ValueError("optimize_newton_ensemble: form '{}' is none of 'workgroup', 'launches', 'auto'".format(form))
    if krylov not in ("never", "auto", "any"):
        raise ValueError("optimize_newton_ensemble: krylov '{}' is neither 'never' nor 'auto' nor 'any'".format(krylov))
    if krylov == "auto" and form == "launches":
        raise ValueError("optimize_newton_ensemble: krylov '{}' with form 'launches' (the hand-over to GCR runs inside the "
                         "one-workgroup solve launch: form 'workgroup')".format(krylov))
    linsolver = getattr(args, "linsolver", "direct")
    if linsolver not in ("direct", "multigrid"):
        raise ValueError("optimize_newton_ensemble: linsolver '{}' (the one-workgroup Newton solves serve 'direct' and "
                         "'multigrid')".format(linsolver))
    if linearize not in ("batched", "members"):
        raise ValueError("optimize_newton_ensemble: linearize '{}' ('batched' or 'members')".format(linearize))
    if getattr(args, "linsolver_damp", 0) or getattr(args, "linsolver_dampdiag", 0):
        raise ValueError("optimize_newton_ensemble: damping (linsolver_damp / linsolver_dampdiag) is not served: the cycles "
                         "solve M d = r, which has the solution of the normal equations only without it")
    refused = dict(poisson=None, stencil=None)  # per route the first (member, reason) it refuses while the other admits
    launches = dict(refused=None, needed=form == "launches")  # (form 'launches' / 'auto': what the batched launches say)
    launches["why"] = None  # (form 'auto': the first (member, reason) for which the one-workgroup form does not serve)

    def describe(b, problem, state, refuse):
        kind = _plain_field(b, problem, state, refuse)
        cshape, dtype = kind["cshape"], kind["dtype"]
        npdt = np.float64 if dtype == torch.float64 else np.float32
        if form != "workgroup":
            reason = fused.newton_launches_refusal(cshape, dtype)
            if reason is not None and form == "launches":
                refuse(b, reason)
            if reason is not None and launches["refused"] is None:
                launches["refused"] = (b, reason)
            if form == "launches":
                return kind
        # (which route runs is known only once the operators are probed: a member that neither admits is refused here, one
        # that a single route refuses once the route is known -- still before any state changes)
        reasons = dict(poisson=fused.newton_refusal(cshape, [npdt(v) ** 2 for v in kind["spacing"]], dtype),
                       stencil=fused.newton_stencil_refusal(cshape, dtype))
        if None not in reasons.values():
            if form == "auto" and launches["refused"] is None:  # (no one-workgroup route: the batched launches serve it)
                launches["needed"] = True
                launches["why"] = launches["why"] or (b, reasons["poisson"])
                return kind
            refuse(b, reasons["poisson"] if form == "workgroup" else "{}; as batched launches: {}".format(
                reasons["poisson"], launches["refused"][1]))
        for route, reason in reasons.items():
            if reason is not None and refused[route] is None:
                refused[route] = (b, reason)
        return kind

    kind, refuse = _check_members("optimize_newton_ensemble", problems, states, describe)

    def keep_krylov():
        """form 'auto' that needs the batched launches does not drop the option silently (known from the shapes alone
        before the operators are probed, from the route's refusal after)."""
        if launches["needed"] and krylov == "auto":
            refuse(launches["why"][0], "{}; the batched launches that serve such members have no hand-over to GCR (krylov "
                   "'{}')".format(launches["why"][1], krylov))

    keep_krylov()
    evaluators = []
    for problem, state in zip(problems, states):
        problem.recognise(state)
        ev = getattr(problem, "_fused", None)
        evaluators.append(ev if ev is not None and ev.nlvl == 1 else None)
    route = "stencil" if any(ev is None for ev in evaluators) else "poisson"
    if form == "auto" and refused[route] is not None and launches["refused"] is None:
        launches["needed"] = True  # (the one-workgroup route these operators take refuses a member)
        launches["why"] = launches["why"] or refused[route]
    keep_krylov()
    if launches["needed"]:
        route = "stencil"
    elif refused[route] is not None:
        refuse(*refused[route])
    ran = "launches" if launches["needed"] else "workgroup"
    options = dict()  # (of the solver's constructor)
    hierarchy = gmg.EnsembleLaunchGMG if ran == "launches" else gmg.EnsembleGMG
    if krylov != "never":
        if ran == "launches":  # (krylov 'any': the hand-over across the batched launches; 'auto' was refused above)
            hierarchy = gmg.EnsembleLaunchKrylovGMG
        else:
            options["krylov"] = "auto"
        reason = _krylov_memory_refusal(len(problems), kind["cshape"], kind["dtype"], kind["device"], gmg.EnsembleGMG.krylov_m)
        if reason is not None:
            raise ValueError("optimize_newton_ensemble: " + reason)
    if route == "poisson":  # (one launch per epoch: the whole Newton step on the packed iterate and right-hand sides)
        ev = evaluators[0]
        solver = gmg.EnsembleGMG(ev.cshape, ev.h2, ev.dtype, ev.device, len(evaluators), **options)
        rhs = torch.stack([e.rhs.reshape(ev.cshape) for e in evaluators])

        def step(u, first, tol, maxcycles):  # (no linearisation: nothing to report)
            solver.newton_step(u, rhs, tol=tol, maxcycles=maxcycles)
    else:
        solver, step = _stencil_route(args, problems, states, kind, linearize, time_linearize, hierarchy, options)
    return _newton_loop(args, problems, states, callback, linsolver, kind["dtype"], route, solver, step, ran)


def _krylov_memory_refusal(nbatch, cshape, dtype, device, m):
    """Why the work memory that krylov='auto' adds -- B (2 m + 2) finest-level vectors: iterate, residual, m directions and
    their images per member -- does not fit the free memory of `device`, or None."""
    need = nbatch * (2 * m + 2) * math.prod(cshape) * torch.empty((), dtype=dtype).element_size()
    if device is not None and torch.device(device).type == "cuda":
        free = torch.cuda.mem_get_info(device)[0]
        if need > free:
            return "krylov 'auto' adds {} members x {} vectors x {} cells = {} bytes of work memory, {} bytes of device " \
                   "memory are free".format(nbatch, 2 * m + 2, math.prod(cshape), need, free)
    return None


def _stencil_route(args, problems, states, kind, linearize="batched", timed=False, hierarchy=gmg.EnsembleGMG, options=None):
    """(solver, step) of the route for members that are not all the Poisson operator (the docstring of
    `optimize_newton_ensemble`); the members have passed its checks, `kind` is what they share.  Linearises once here,
    before any state changes: a member that has no stencil Jacobian is named first.  Without an epoch to run, no solver.
    hierarchy: the class whose `from_coeffs` makes the solver (gmg.EnsembleGMG; for form 'launches' gmg.EnsembleLaunchGMG or
    gmg.EnsembleLaunchKrylovGMG);
    options: further keywords of it (krylov).
    step returns (Jacobian launches made, the pair of events around the linearisation or None)."""
    nb, cshape, dtype, device = len(problems), kind["cshape"], kind["dtype"], kind["device"]
    ndim = len(cshape)
    stage = torch.empty((nb, 2 * ndim + 1) + cshape, dtype=dtype, device=device)  # (the Jacobians of the first step)
    r = torch.empty((nb,) + cshape, dtype=dtype, device=device)
    d = torch.zeros_like(r)

    def members(target):
        """r[b] = f_b(u_b) and target[b] = the coefficient arrays of member b's Jacobian, member by member."""
        for b, (problem, state) in enumerate(zip(problems, states)):
            vector, matrix = problem.linearize_device(state)
            coeffs = gmg.recognise_stencil(matrix)
            if coeffs is None or tuple(coeffs.shape[1:]) != cshape:
                raise ValueError("optimize_newton_ensemble: member {}: its Jacobian is not a (2 d + 1)-point stencil of one "
                                 "cell-centred plain Field".format(b))
            target[b].copy_(coeffs)
            r[b].view(-1).copy_(vector.reshape(-1))
        return nb

    batched = None

    def linearise(target):
        nonlocal batched
        events = None
        if timed:
            events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            events[0].record()
        if linearize == "members":
            launches = members(target)
        else:
            if batched is None:  # (the members' plan: traced once per list of problems, kept with them)
                batched = _held_linearizer(problems, states, kind, "optimize_newton_ensemble")
            launches = batched(states, coeffs=target, values=r)[2].launches
        if timed:
            events[1].record()
        return launches, events

    solver, first = None, None
    if args.epochs > args.epoch_start:
        first = linearise(stage)
        solver = hierarchy.from_coeffs(stage, **(options or dict()))
    del stage

    def step(u, is_first, tol, maxcycles):
        made = first
        if not is_first:
            made = linearise(solver.fine)
            solver.rebuild()
        solver.solve(r, d, tol=tol, maxcycles=maxcycles, start=2)  # M_b d_b = r_b, the convention of optimize_newton
        ops.axpy(u.view(-1), d.view(-1), -1.0)                     # u -= d for all members
        return made

    return solver, step


def _jacobians_generated(device):
    """Whether `Problem.eval_operator_grad` takes the generated Jacobian kernel (its own condition) for members on `device`."""
    from . import runtime

    return bool(runtime.enable_trace and int(os.environ.get("ODIL_TRACE_JAC", 1)) and torch.cuda.is_available()
                and device.type == "cuda")


def _stencil_member(b, problem, state, refuse):
    """`describe` of `_check_members` for members of the stencil route alone."""
    from . import fused

    kind = _plain_field(b, problem, state, refuse)
    reason = fused.newton_stencil_refusal(kind["cshape"], kind["dtype"])
    if reason is not None:
        refuse(b, reason)
    return kind


class EnsembleLinearizer:
    """The linearisation of B members of the stencil route, planned once: which members share a launch, where every
    array of the generated Jacobian kernel goes.  Members are traced with the batched form of the Jacobian kernel
    (`stencil_jit.trace_jacobian(batch=True)`); those whose generated sources are equal load one library and are linearised
    by ONE launch of its `k_jac_batch` (stencil_bind.JacobianBatch), which writes f(u) into values[b] and d f / d read into
    the slot of coeffs[b] that `gmg.stencil_slot_plan` names -- no intermediate buffer, no copy.  Members without a
    generated Jacobian (ODIL_TRACE_JAC=0, an operator the generator refuses) or whose reads land twice in one slot go
    through `linearize_device` and `gmg.recognise_stencil` on their own (`single`: {member: reason})."""

    def __init__(self, problems, states, who="linearize_ensemble", kind=None):
        """kind: what `_check_members` returned for these members when the caller has checked them already."""
        def refuse(member, reason):
            raise ValueError("{}: member {}: {}".format(who, member, reason))

        if kind is None:
            kind, refuse = _check_members(who, problems, states, _stencil_member)
        self.who, self.kind, self.problems, self.nb = who, kind, list(problems), len(problems)
        self._plan(states, refuse)

    def _plan(self, states, refuse):
        from . import stencil_jit
        from .stencil_bind import JacobianBatch

        cshape = self.kind["cshape"]
        self.traced, self.plans, self.single = [None] * self.nb, [None] * self.nb, dict()
        self.generated = _jacobians_generated(self.kind["device"])
        for b, (problem, state) in enumerate(zip(self.problems, states)):
            if not self.generated:
                self.single[b] = "no generated Jacobian kernel (tracing or ODIL_TRACE_JAC switched off, or no device)"
                continue
            if any(getattr(type(problem), name, None) is not getattr(Problem, name) for name in ("linearize_device", "eval_operator_grad")):
                self.single[b] = "no generated Jacobian kernel: the member linearises itself (its own `linearize_device`)"
                continue
            traced = stencil_jit.trace_jacobian(problem, state, batch=True)
            if traced is None:
                self.single[b] = "no generated Jacobian kernel for its operator"
                continue
            try:
                plan = gmg.stencil_slot_plan(traced.cg.jac_items, traced.G, {k: f.loc for k, f in state.fields.items()})
                if tuple(traced.G) != cshape:
                    raise ValueError("its residual lives on a grid {}".format(tuple(traced.G)))
            except ValueError as e:
                refuse(b, "its Jacobian is not a (2 d + 1)-point stencil of one cell-centred plain Field ({})".format(e))
            if plan.single is not None:
                self.single[b] = plan.single
                continue
            self.traced[b], self.plans[b] = traced, plan
        by_lib = dict()
        for b, traced in enumerate(self.traced):
            if traced is not None:
                by_lib.setdefault(traced.lib_path, []).append(b)
        self.groups = list(by_lib.values())
        self.batches = [JacobianBatch([self.traced[b] for b in group]) for group in self.groups]
        self._tables = None  # ((address and strides of the buffers), per group the pointer table of its launch)
        # slots that no read of a member writes: zero arrays, filled in one launch per slot for all members that miss it
        self.missing = []
        for slot in range(2 * len(cshape) + 1):
            who = [b for b, plan in enumerate(self.plans) if plan is not None and slot in plan.missing]
            if who:
                self.missing.append((slot, slice(None) if len(who) == self.nb else torch.tensor(who, device=self.kind["device"])))

    def __call__(self, states, coeffs=None, values=None):
        """(values [B, *cshape], coeffs [B, 2 d + 1, *cshape], info) at `states`; coeffs / values: the buffers to write
        (each member's arrays contiguous; e.g. `gmg.EnsembleGMG.fine`), allocated when None.  Slots that no read of a
        member writes are zero-filled, one launch per such slot (the kernel never touches them; on every call: a buffer
        the caller has rewritten cannot be told from the one filled before).
        info.launches: Jacobian launches made, info.groups: the members of each shared launch, info.single: [(member,
        reason)] linearised on their own."""
        kind, nb = self.kind, self.nb
        cshape, ndim = kind["cshape"], len(kind["cshape"])
        if len(states) != nb:
            raise ValueError("{}: {} problems with {} states".format(self.who, nb, len(states)))
        if coeffs is None:
            coeffs = torch.empty((nb, 2 * ndim + 1) + cshape, dtype=kind["dtype"], device=kind["device"])
        if values is None:
            values = torch.empty((nb,) + cshape, dtype=kind["dtype"], device=kind["device"])
        for name, t, want in (("coeffs", coeffs, (nb, 2 * ndim + 1) + cshape), ("values", values, (nb,) + cshape)):
            if tuple(t.shape) != want or t.dtype != kind["dtype"] or t.device != kind["device"]:
                raise ValueError("{}: `{}` is not a {} tensor of shape {} on {}".format(self.who, name, kind["dtype"], want,
                                                                                     kind["device"]))
        for slot, who in self.missing:
            coeffs[who, slot] = 0
        ident = tuple((t.data_ptr(), tuple(t.stride())) for t in (coeffs, values))
        if self._tables is None or self._tables[0] != ident:  # (the pointers of these buffers: once, not B (2 d + 2) views per call)
            self._tables = (ident, [batch.pointer_table(
                [[values[b] if slot is None else coeffs[b, slot] for slot in self.plans[b].slots] for b in group])
                for group, batch in zip(self.groups, self.batches)])
        for group, batch, table in zip(self.groups, self.batches, self._tables[1]):
            batch.launch([states[b] for b in group], table)
        for b in sorted(self.single):
            vector, matrix = self.problems[b].linearize_device(states[b])
            found = gmg.recognise_stencil(matrix)
            if found is None or tuple(found.shape[1:]) != cshape:
                raise ValueError("{}: member {}: its Jacobian is not a (2 d + 1)-point stencil of one cell-centred plain "
                                 "Field".format(self.who, b))
            coeffs[b].copy_(found)
            values[b].view(-1).copy_(vector.reshape(-1))
        info = argparse.Namespace(launches=len(self.groups) + len(self.single), groups=[list(g) for g in self.groups],
                                  single=[(b, self.single[b]) for b in sorted(self.single)])
        return values, coeffs, info


def linearize_ensemble(problems, states, coeffs=None, values=None):
    """f_b(u_b) and the Jacobian's coefficient arrays of B members of the stencil route of `optimize_newton_ensemble`, all
    members whose operators generate the same kernels in ONE launch: (values [B, *cshape], coeffs [B, 2 d + 1, *cshape] in
    the layout of `gmg.stencil_coefficients`, info) -- `EnsembleLinearizer`, which this makes on the first call for a list
    of problems and reuses afterwards (kept on problems[0]; traced operators that no longer match the states are traced
    again).  Members are checked as the driver checks them (`fused.newton_stencil_refusal`: one plain cell-centred `Field`,
    same cshape, spacing, dtype and device); a refusal is a ValueError naming the first offending member, before any
    operator is traced."""
    kind, _ = _check_members("linearize_ensemble", problems, states, _stencil_member)
    return _held_linearizer(problems, states, kind, "linearize_ensemble")(states, coeffs=coeffs, values=values)


def _held_linearizer(problems, states, kind, who):
    """The `EnsembleLinearizer` of these (checked) members: the one kept on problems[0] when it was planned for the same
    problem objects, the same kind and states its traced operators still match, else a new one."""
    held = getattr(problems[0], "_ensemble_linearizer", None)
    if not (held is not None and held.kind == kind and held.generated == _jacobians_generated(kind["device"])
            and len(held.problems) == len(problems) and all(p is q for p, q in zip(held.problems, problems))
            and all(t is None or t.matches(state) for t, state in zip(held.traced, states))):
        held = problems[0]._ensemble_linearizer = EnsembleLinearizer(problems, states, who=who, kind=kind)
    held.who = who
    return held


def _newton_loop(args, problems, states, callback, linsolver, dtype, route, solver, step, form="workgroup"):
    """What the Newton routes share.  route: "poisson" / "stencil"; form: "workgroup" / "launches", reported as
    optinfo.form; solver: its gmg.EnsembleGMG or gmg.EnsembleLaunchGMG (None only when no epoch
    runs); step(u, first, tol, maxcycles) advances the packed iterate u [B, *cshape] by one Newton step of every member
    (first: at args.epoch_start) and leaves solver.outcome / status(b) behind; it returns None or (Jacobian launches it
    made, None or the pair of timing events around its linearisation)."""
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
    handover = np.full((nb, nepochs), -1, dtype=np.int64)
    residuals = np.zeros((nb, nepochs))
    launches, events = np.zeros(nepochs, dtype=np.int64), []
    next_active = getattr(callback, "next_active", None) if callback else None
    due = None
    if callback:
        report(args.epoch_start, False)
        due = next_active(args.epoch_start) if next_active else args.epoch_start + 1
    for epoch in range(args.epoch_start, args.epochs):
        made = step(u, epoch == args.epoch_start, tol, maxcycles)
        k = epoch - args.epoch_start
        if made is not None:
            launches[k] = made[0]
            events.append(made[1])
        cycles[:, k] = solver.outcome[:, 0]
        if solver.outcome.shape[1] > 2:  # (a solver with the hand-over to GCR: the cycle it happened before, or -1)
            handover[:, k] = solver.outcome[:, 2]
        residuals[:, k] = [solver.status(b)["residual"] for b in range(nb)]
        if getattr(args, "linsolver_verbose", 0):
            util.printlog([solver.status(b) for b in range(nb)])
        if callback and epoch + 1 >= due:
            report(epoch + 1, True)
            due = next_active(epoch + 1) if next_active else epoch + 2
    arrays = [problem.domain.arrays_from_state(state) for problem, state in zip(problems, states)]
    linearize_ms = None
    if events and all(pair is not None for pair in events):
        torch.cuda.synchronize()
        linearize_ms = np.array([pair[0].elapsed_time(pair[1]) for pair in events])
    return arrays, argparse.Namespace(epochs=args.epochs, evals=nepochs, cycles=cycles, residuals=residuals, solver=solver,
                                      route=route, form=form, linearize_launches=launches, linearize_ms=linearize_ms,
                                      handover=handover)
