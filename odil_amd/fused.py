"""Recognition of affine stencil operators and their fused evaluation.

A user `operator(ctx)` is arbitrary Python over `mod`, so only framework-owned arithmetic
can be hand-written generically.  But an operator that is AFFINE in a single cell-centred
field is completely determined by its per-shift Jacobian coefficient arrays (what
`Problem.eval_operator_grad` returns, reference core.py:1313-1361) and its value at one
state.  `detect()` evaluates the user's operator through the generic path at two probe
states; if (a) the coefficient arrays do not depend on the state, (b) they equal the
coefficients of the zero-Dirichlet Laplacian of the Poisson example (reference
examples/poisson/poisson.py:57-113) for this domain's steps, and (c) the operator did not
read `ctx.tracers`, then `fu = Lap(u) - rhs_eff` with `rhs_eff = Lap(u_A) - f(u_A)`, and
the problem is routed to the fused HIP kernels (residual + loss, adjoint, multigrid
synthesis / P^T chain).  Anything else keeps the generic path.  Like `jax.jit` in the
reference (core.py:1107), this bakes `extra` in at first evaluation.  ODIL_FUSE=0 disables it.
"""

import math

import numpy as np
import torch

from . import ops


class PoissonEvaluator:
    """Fused loss + gradient of `fu = Lap(u) - rhs` for a (multigrid) cell-centred unknown."""

    def __init__(self, cshape, shapes, rhs, h2, name="", dtype=torch.float64, device=None):
        self.cshape = tuple(cshape)
        self.ndim = len(cshape)
        self.loc = "c" * self.ndim
        self.shapes = [tuple(s) for s in shapes]
        self.nlvl = len(shapes)
        self.sizes = [math.prod(s) for s in self.shapes]
        self.rhs = rhs
        self.h2 = list(h2)
        self.names = [name]
        self.dtype, self.device = dtype, device
        self.npdt = np.float64 if dtype == torch.float64 else np.float32
        n = sum(self.sizes)
        self.g = torch.zeros(n, dtype=dtype, device=device)
        self.gw = [t.view(s) for t, s in zip(self.g.split(self.sizes), self.shapes)]
        self._u = None  # synthesised field, allocated on first use (the fused residual does not need it)
        self.fu = torch.empty(self.cshape, dtype=dtype, device=device)
        self.loss = torch.zeros((), dtype=dtype, device=device)
        self.work = ([None] + [torch.empty(s, dtype=dtype, device=device) for s in self.shapes[1:-1]] + [None])[
            : self.nlvl
        ]
        self.scale = self.npdt(2) / self.npdt(self.fu.numel())
        self.timers = None  # (measurement: event pairs around the launches of every evaluation, see loss_grad_arrays)
        import os

        # last prolongation fused into the residual (u never stored): 3-D, even extents, >= 2 levels
        self.synth_residual = (
            self.ndim == 3 and self.nlvl >= 2 and all(s % 2 == 0 and s >= 4 for s in self.cshape)
            and tuple(self.shapes[1]) == tuple(s // 2 for s in self.cshape)
            and bool(int(os.environ.get("ODIL_SYNTH_RESIDUAL", 1))))
        # stencil adjoint, first transposed prolongation and the Adam updates of both levels in one launch
        self.fuse_transpose = (
            self.ndim == 3 and self.nlvl >= 2 and ops.adjoint_transpose_supported(self.cshape)
            and tuple(self.shapes[1]) == tuple(s // 2 for s in self.cshape)
            and bool(int(os.environ.get("ODIL_FUSE_TRANSPOSE", 1))))

    def adjoint_and_transposes(self, arrays, adam, tic=lambda name: None, toc=lambda b: None):
        """grads (and, with `adam`, the update of every level) from the residual in self.fu."""
        if adam is not None:
            ml, vl, alpha, omb1, omb2, eps = adam
        if adam is not None and self.fuse_transpose:
            # stencil adjoint + first P^T + the updates of both levels in one launch: the finest-level gradient
            # never goes through memory and is not stored (gw[0] is left as it was).  Without the updates the
            # separate kernels are faster (the one-pass kernel is bound by its LDS / VALU phases at two
            # workgroups per CU: 1.6 ms against 0.54 + 0.45 ms at 512^3), so gradients alone keep them.
            b = tic("adjoint_transpose")
            ops.poisson_adjoint_transpose(self.fu, self.h2, self.scale, self.gw[1], g0=None,
                                          adam0=(arrays[0], ml[0], vl[0]), adam1=(arrays[1], ml[1], vl[1]),
                                          alpha=alpha, one_minus_b1=omb1, one_minus_b2=omb2, eps=eps)
            toc(b)
            if self.nlvl > 2:
                b = tic("mg_synth_adj")
                ops.mg_synth_adj_adam(self.gw[1], self.shapes[1:], self.loc, self.gw[1:], arrays[1:], ml[1:], vl[1:],
                                      alpha, omb1, omb2, eps)
                toc(b)
            return
        b = tic("adjoint")
        if adam is not None:
            ops.poisson_adjoint_adam(self.fu, self.h2, self.scale, self.gw[0], arrays[0], ml[0], vl[0], alpha, omb1,
                                     omb2, eps)
        else:
            ops.poisson_adjoint(self.fu, self.h2, self.scale, out=self.gw[0])
        toc(b)
        if self.nlvl > 1:
            b = tic("mg_synth_adj")
            if adam is not None:
                ops.mg_synth_adj_adam(self.gw[0], self.shapes, self.loc, self.gw, arrays, ml, vl, alpha, omb1, omb2, eps)
            else:
                ops.mg_synth_adj(self.gw[0], self.shapes, self.loc, grads=self.gw)
            toc(b)

    @property
    def u(self):
        if self._u is None and self.nlvl > 1:
            self._u = torch.empty(self.cshape, dtype=self.dtype, device=self.device)
        return self._u

    def loss_grad_arrays(self, arrays, timers=None, adam=None):
        """arrays: level arrays fine -> coarse.  Returns (loss 0-d tensor, grads views of one buffer).
        adam = (m_levels, v_levels, alpha, 1-b1, 1-b2, eps): also apply the Adam update of EVERY
        level array inside the launch that forms its gradient (adjoint for level 0, the P^T
        chain for the others); no separate optimizer launch is needed then."""

        timers = timers if timers is not None else self.timers

        def tic(name):
            if timers is None:
                return None
            a, b = timers.section(name)
            a.record()
            return b

        def toc(b):
            if b is not None:
                b.record()

        if self.synth_residual:
            b = tic("mg_synth")
            if self.nlvl > 2:
                coarse = ops.mg_synth(arrays[1:], self.loc, work=[None] + self.work[2:], out=self.work[1])
            else:
                coarse = arrays[1]
            toc(b)
            u = None
        elif self.nlvl > 1:
            b = tic("mg_synth")
            u = ops.mg_synth(arrays, self.loc, work=self.work, out=self.u)
            toc(b)
        else:
            u = arrays[0]
        b = tic("residual")
        if self.synth_residual:
            ops.poisson_residual_synth(coarse, arrays[0], self.rhs, self.h2, fu=self.fu, loss=self.loss)
        else:
            ops.poisson_residual(u, self.rhs, self.h2, fu=self.fu, loss=self.loss)
        toc(b)
        self.adjoint_and_transposes(arrays, adam, tic, toc)
        return self.loss, self.gw

    def eval_loss_grad(self, state):
        (field,) = state.fields.values()
        arrays = [t.array for t in field.terms] if hasattr(field, "terms") else [field.array]
        arrays = [a if a.is_contiguous() else a.contiguous() for a in arrays]
        loss, grads = self.loss_grad_arrays(arrays)
        return loss, list(grads), [loss], self.names, [torch.sqrt(loss)]


    def eval_loss_grad_adam(self, state, m, v, alpha, omb1, omb2, eps):
        """eval_loss_grad + the Adam step of every level inside the launches that form the
        gradients.  Returns (..., done=nlvl) or None when this configuration cannot fuse."""
        import os

        if self.nlvl < 2 or not int(os.environ.get("ODIL_FUSE_ADAM0", 1)):
            return None
        (field,) = state.fields.values()
        arrays = [t.array for t in field.terms]
        if not all(a.is_contiguous() for a in list(arrays) + list(m) + list(v)):
            return None
        loss, grads = self.loss_grad_arrays(arrays, adam=(m, v, alpha, omb1, omb2, eps))
        return loss, list(grads), [loss], self.names, [torch.sqrt(loss)], self.nlvl


    # ---- whole epochs in one launch (small 1-D / 2-D problems) --------------------------------------------------------------
    # ONE workgroup walks the epoch (odil_poisson_small_epochs) when the state fits its LDS (1-D N <= 1024 in float64, 2-D
    # 32^2; twice that in float32) -- 15 us per epoch at 1-D N = 256 against 58 replayed as a hipGraph -- and, from
    # global memory, for 1-D grids up to this many cells (N = 4096: 40 us against 82).  Beyond, the separate kernels win:
    # one workgroup is one CU's worth of bandwidth and a memory round trip per phase.
    small_max_cells = 4096
    small_force = False  # (tests: the global-memory form on any 1-D / 2-D problem)

    def small_plan(self, arrays, m, v):
        """The packed vectors (x, m, v, g) when `arrays` / m / v are the level slices of packed vectors in level order and
        the problem is small enough for one workgroup; None otherwise."""
        if len(arrays) != self.nlvl or small_refusal(self.shapes, self.dtype, self.small_force, self.small_max_cells):
            return None

        def packed(levels):
            base, item, off = levels[0].data_ptr(), levels[0].element_size(), 0
            for t, size in zip(levels, self.sizes):
                if not t.is_contiguous() or t.numel() != size or t.dtype != self.dtype or t.data_ptr() != base + off * item:
                    return None
                off += size
            return levels[0]

        heads = [packed(list(levels)) for levels in (arrays, m, v, self.gw)]
        return None if any(hd is None for hd in heads) else heads

    def small_epochs(self, heads, alphas, losses, norms, omb1, omb2, eps):
        """alphas.numel() Adam epochs in ONE launch on the packed vectors of `small_plan`; the loss every epoch evaluated
        (and its square root) land in `losses` / `norms` (device tensors like `alphas`)."""
        if self.__dict__.get("_small_u") is None:
            self._small_u = torch.empty(sum(self.sizes), dtype=self.dtype, device=self.device)
        ops.poisson_small_epochs(heads[0], heads[1], heads[2], heads[3], self._small_u, self.fu, self.rhs, self.shapes,
                                 self.h2, alphas, omb1, omb2, eps, losses, norms)


class _Members:
    """What every ensemble class answers before it holds anything: whether these evaluators run side by side."""

    shape_refusal = None  # (evaluator) -> reason or None: the predicate of the class's form

    @classmethod
    def refusal(cls, evaluators):
        """(member, reason) of the first member that keeps these evaluators from running as one ensemble, else None."""
        if not evaluators:
            return 0, "an ensemble needs at least one member"
        first = evaluators[0]
        for b, ev in enumerate(evaluators):
            if not isinstance(ev, PoissonEvaluator):
                return b, "the operator is not the recognised Poisson stencil"
            reason = cls.shape_refusal(ev)
            if reason is not None:
                return b, reason
            for what in ("cshape", "shapes", "dtype", "device"):
                if getattr(ev, what) != getattr(first, what):
                    return b, "{} {} differs from member 0's {}".format(what, getattr(ev, what), getattr(first, what))
            if [float(a) for a in ev.h2] != [float(a) for a in first.h2]:
                return b, "grid spacing differs from member 0's"
        return None


class PoissonEnsemble(_Members):
    """B recognised Poisson problems of one shape side by side: packed [B, unknowns] state, moments, gradient and synthesis
    scratch, [B, cells] residuals and right-hand sides, and whole Adam epochs of every member in ONE launch with one
    workgroup per member (odil_poisson_small_epochs_batch).  Member b computes what `PoissonEvaluator.small_epochs`
    computes for it alone, bit for bit: the kernel runs the same per-workgroup code on offset pointers."""

    def __init__(self, evaluators):
        from ._lib import i64, load

        reason = self.refusal(evaluators)
        if reason is not None:
            raise ValueError("ensemble member {}: {}".format(*reason))
        ev = evaluators[0]
        self.shapes, self.sizes, self.h2, self.dtype, self.device = ev.shapes, ev.sizes, ev.h2, ev.dtype, ev.device
        self.nbatch, self.total, self.cells = len(evaluators), sum(ev.sizes), ev.sizes[0]
        self.names = [e.names for e in evaluators]
        packed = lambda: torch.zeros((self.nbatch, self.total), dtype=self.dtype, device=self.device)
        self.x, self.m, self.v, self.g = packed(), packed(), packed(), packed()
        self.u = torch.empty_like(self.x)
        self.fu = torch.empty((self.nbatch, self.cells), dtype=self.dtype, device=self.device)
        self.rhs = torch.stack([e.rhs.reshape(-1) for e in evaluators])
        npart = int(load().odil_poisson_small_epochs_partials(i64(self.shapes[0]), ev.ndim, self.x.element_size()))
        self.partials = torch.empty((self.nbatch, npart), dtype=torch.float64, device=self.device)

    shape_refusal = staticmethod(lambda ev: small_refusal(ev.shapes, ev.dtype, ev.small_force, ev.small_max_cells))

    def levels(self, packed, member):
        """The level arrays of one member: views of a row of a packed [B, unknowns] tensor."""
        return [t.view(s) for t, s in zip(packed[member].split(self.sizes), self.shapes)]

    def epochs(self, alphas, losses, norms, omb1, omb2, eps):
        """losses.shape[1] Adam epochs of every member in ONE launch.  alphas: [B, E] step sizes, or [E] shared by all
        members; the loss every epoch evaluated and its square root land in losses / norms [B, E] (device tensors)."""
        ops.poisson_small_epochs_batch(self.x, self.m, self.v, self.g, self.u, self.fu, self.rhs, self.shapes, self.h2,
                                       alphas, omb1, omb2, eps, losses, norms, self.partials)


class BatchedLaunches(_Members):
    """What the ensembles that run as batched launches share (PoissonLaunchEnsemble, PoissonVolumeEnsemble,
    TracedLaunchEnsemble): level-major [B, *shape] storage and epochs one at a time -- the interface
    `AdamNativeOptimizer.run_ensemble` drives; for the Poisson forms also the refusal of members that differ, their
    residuals and right-hand sides."""

    graphable = True  # epochs may be replayed as a captured graph (no launch argument changes between epochs)

    def __init__(self, evaluators, pad, levels_refusal):
        """What both Poisson forms hold: x, m, v, g (one [B, *shape] tensor per level), fu, rhs, loss and norm.
        levels_refusal(shapes, nbatch, dtype): the library's answer why a transfer level of the batch would not run the
        kernel that level of a single member runs, or None -- asked before the first launch."""
        reason = self.refusal(evaluators)
        if reason is not None:
            raise ValueError("ensemble member {}: {}".format(*reason))
        ev = evaluators[0]
        reason = levels_refusal(ev.shapes, len(evaluators), ev.dtype)
        if reason is not None:
            raise ValueError("ensemble of {} members: {}".format(len(evaluators), reason))
        self.h2, self.scale = ev.h2, float(ev.scale)
        self._allocate(ev.shapes, ev.dtype, ev.device, [e.names for e in evaluators], pad)
        self.fu, self.rhs = self.members(self.cshape, pad), self.members(self.cshape, pad)
        self.rhs.copy_(torch.stack([e.rhs.reshape(self.cshape) for e in evaluators]))

    def _allocate(self, shapes, dtype, device, names, pad=0, loc=None, nfields=1):
        """The level-major state of len(names) members of these level shapes: x, m, v, g, loss and norm.  pad: extra
        elements between the members of m[0] and v[0].  loc: the location string of a member's arrays (default: all axes
        cell-centred); nfields: grid unknowns per member, stacked on the member axis (`nrows` = nfields B rows per level
        tensor, row f B + b)."""
        self.shapes, self.dtype, self.device = [tuple(s) for s in shapes], dtype, device
        self.sizes = [math.prod(s) for s in self.shapes]
        self.cshape, self.ndim = self.shapes[0], len(self.shapes[0])
        self.loc = "." + (loc or "c" * self.ndim)
        self.nbatch, self.nlvl, self.cells = len(names), len(self.shapes), self.sizes[0]
        self.nfields, self.nrows, self.total = nfields, nfields * self.nbatch, nfields * sum(self.sizes)
        self.names = names
        level = lambda wide0=0: [self.members(s, wide0 if l == 0 else 0) for l, s in enumerate(self.shapes)]
        self.x, self.m, self.v, self.g = level(), level(pad), level(pad), level()
        self.loss, self.norm = (torch.zeros(self.nbatch, dtype=self.dtype, device=self.device) for _ in range(2))

    def members(self, shape, wide=0):
        """Zeroed [B, *shape] tensor ([nfields B, *shape] where the members' grid unknowns are stacked) with `wide` extra
        elements between its contiguous members."""
        cells = math.prod(shape)
        base = torch.zeros(self.nrows * (cells + wide), dtype=self.dtype, device=self.device)
        strides = [math.prod(shape[k + 1:]) for k in range(len(shape))]
        return base.as_strided((self.nrows,) + tuple(shape), [cells + wide] + strides)

    def levels(self, packed, member):
        """The level arrays of one member: views of the [B, *shape] level tensors."""
        return [t[member] for t in packed]

    def blocks(self, packed):
        """`packed` (x, m, v or g) as [B, size] views in the order of the members' `arrays_from_state`: what an optimizer
        on member-major [B, n] vectors copies from and to, block by block."""
        return [t.view(self.nbatch, -1) for t in packed]

    def loss_grad(self):
        """The launches of `epoch` WITHOUT any update (what an optimizer that is not Adam drives: L-BFGS-B in lock-step):
        the [B] losses at self.x land in self.loss, the gradient of every level in self.g; x, m and v stay as they are.
        Member b gets the bits of its single gradient evaluation."""
        raise NotImplementedError

    def _transposes(self):
        """The gradients of the levels >= 1 from g[0]: the chain of `epoch` without x, m and v, on the levels the
        ensemble's constructor has asked the library about."""
        if self.nlvl > 1:
            ops.mg_synth_adj_adam_members(self.g[0], self.shapes, self.loc[1:], self.g)

    def epochs(self, alphas, losses, norms, omb1, omb2, eps):
        """losses.shape[1] epochs (the interface of PoissonEnsemble.epochs).  alphas: [B, E], or [E] shared by all members."""
        for e in range(losses.shape[1]):
            self.epoch(alphas[..., e].contiguous().view(-1), omb1, omb2, eps)
            torch.sqrt(self.loss, out=self.norm)
            losses[:, e].copy_(self.loss)
            norms[:, e].copy_(self.norm)


class PoissonLaunchEnsemble(BatchedLaunches):
    """B recognised Poisson problems of one shape and ANY 1-D / 2-D size side by side, as batched launches: an epoch is the
    launches of `PoissonEvaluator.loss_grad_arrays(adam=...)` for a 2-D problem -- synthesis, residual + loss, adjoint +
    update of level 0, transposed prolongations + updates of the other levels -- each covering all B members
    (odil_mg_synth on [B, *shape] arrays, odil_poisson_residual_batch, odil_poisson_adjoint_adam_batch,
    odil_mg_synth_adj_adam_members).  Level-major storage: x, m, v, g are lists of one [B, *shape] tensor per level.  Member
    b computes what its single run computes, bit for bit: the same per-thread arithmetic, the same summation order.
    pad: extra elements between the members of the arrays that only the stencil kernels touch (fu, rhs, m[0], v[0])."""

    def __init__(self, evaluators, pad=0):
        super().__init__(evaluators, pad, _levels_refusal)
        self.u = self.members(self.cshape)
        self.work = ([None] + [self.members(s) for s in self.shapes[1:-1]] + [None])[: self.nlvl]
        npart = ops.poisson_batch_partials(self.cshape, self.dtype)
        self.partials = torch.empty((self.nbatch, npart), dtype=torch.float64, device=self.device)

    shape_refusal = staticmethod(lambda ev: launches_refusal(ev.shapes, ev.dtype))

    def epoch(self, alphas, omb1, omb2, eps):
        """One Adam epoch of every member; alphas: DEVICE step sizes, [B] or one element shared by all members.  The [B]
        losses the epoch evaluated (before its update) land in self.loss."""
        ops.mg_synth(self.x, self.loc, work=self.work, out=self.u)
        ops.poisson_residual_batch(self.u, self.rhs, self.h2, self.fu, self.loss, self.partials)
        ops.poisson_adjoint_adam_batch(self.fu, self.h2, self.scale, self.g[0], self.x[0], self.m[0], self.v[0], alphas, omb1,
                                       omb2, eps)
        ops.mg_synth_adj_adam_members(self.g[0], self.shapes, self.loc[1:], self.g, self.x, self.m, self.v, alphas, omb1, omb2,
                                      eps)

    def loss_grad(self):
        ops.mg_synth(self.x, self.loc, work=self.work, out=self.u)
        ops.poisson_residual_batch(self.u, self.rhs, self.h2, self.fu, self.loss, self.partials)
        ops.poisson_adjoint_batch(self.fu, self.h2, self.scale, self.g[0])
        self._transposes()


class PoissonVolumeEnsemble(BatchedLaunches):
    """B recognised 3-D Poisson problems of one shape side by side, as batched launches: an epoch is the launches of
    `PoissonEvaluator.loss_grad_arrays(adam=...)` for a 3-D problem through its separate kernels -- synthesis of the
    coarse levels, residual with the last prolongation fused in + loss, adjoint + update of level 0, transposed
    prolongations + updates of the other levels -- each covering all B members (odil_mg_synth on [B, *shape] arrays,
    odil_poisson_residual_synth_batch, odil_poisson_adjoint_adam_volumes, odil_mg_synth_adj_adam_members).  Level-major
    storage as in PoissonLaunchEnsemble.  Member b computes what its single run computes, bit for bit -- also where the
    single run takes the one-pass adjoint + first transpose launch, which equals the separate kernels bit for bit.
    pad: extra elements between the members of the arrays that only the stencil kernels touch (fu, rhs, m[0], v[0])."""

    def __init__(self, evaluators, pad=0):
        super().__init__(evaluators, pad, _levels_refusal)
        # synthesis scratch of the levels 1 ... nlvl - 2 (level 1: the coarse operand of the residual)
        self.work = [None] + [self.members(s) for s in self.shapes[1:-1]] + [None]
        nsums, npart = ops.residual_synth_batch_workspace(self.shapes[1])
        self.sums = torch.empty((self.nbatch, nsums), dtype=torch.float64, device=self.device)
        self.partials = torch.empty((self.nbatch, npart), dtype=torch.float64, device=self.device)

    shape_refusal = staticmethod(lambda ev: volumes_refusal(ev.shapes, ev.dtype))

    def epoch(self, alphas, omb1, omb2, eps):
        """One Adam epoch of every member; alphas: DEVICE step sizes, [B] or one element shared by all members.  The [B]
        losses the epoch evaluated (before its update) land in self.loss."""
        if self.nlvl > 2:
            coarse = ops.mg_synth(self.x[1:], self.loc, work=[None] + self.work[2:], out=self.work[1])
        else:
            coarse = self.x[1]
        ops.poisson_residual_synth_batch(coarse, self.x[0], self.rhs, self.h2, self.fu, self.loss, self.partials, self.sums)
        ops.poisson_adjoint_adam_volumes(self.fu, self.h2, self.scale, self.g[0], self.x[0], self.m[0], self.v[0], alphas,
                                         omb1, omb2, eps)
        ops.mg_synth_adj_adam_members(self.g[0], self.shapes, self.loc[1:], self.g, self.x, self.m, self.v, alphas, omb1, omb2,
                                      eps)

    def loss_grad(self):
        if self.nlvl > 2:
            coarse = ops.mg_synth(self.x[1:], self.loc, work=[None] + self.work[2:], out=self.work[1])
        else:
            coarse = self.x[1]
        ops.poisson_residual_synth_batch(coarse, self.x[0], self.rhs, self.h2, self.fu, self.loss, self.partials, self.sums)
        ops.poisson_adjoint_batch(self.fu, self.h2, self.scale, self.g[0])
        self._transposes()


class _Levels(list):
    """The level tensors of one packed quantity of an ensemble (x, m, v or g) with `.params`: the [B, P] tensor of the
    members' `Array` and `NeuralNet` unknowns beside them."""

    params = None


class TracedLaunchEnsemble(BatchedLaunches):
    """B traced stencil operators of one cell-centred unknown (a `MultigridField` with factors 1, or a plain `Field`: the
    one-level case) on one grid side by side, as batched launches: an epoch is the launches of a single traced run
    (`stencil_jit.TracedOperator.eval_loss_grad` + the optimizer's update), each covering all B members --
      1. `ops.mg_synth` of all levels into u [B, *cshape] (one level: u is x[0]);
      2. the generated forward kernels of all members (`stencil_bind.EpochBatch`: k_fwd_batch, k_final_batch, k_loss_batch),
         ONE launch of each per group of members whose operators generated the same source;
      3. the generated gathers of all members into g[0];
      4. the transposed prolongations with the updates of the levels >= 1 (`ops.mg_synth_adj_adam_members`);
      5. `ops.adam_step_batch` for level 0, after the chain has read g[0] (and after the gathers have re-read their
         sources: for a plain `Field` the source IS x[0]).
    Member b computes what its single run computes, bit for bit.  out [B, 1 + 2 nout_b] per group holds loss, terms and
    norms of its members (`report`); `loss` [B] collects column 0.

    Inverse problems: beside the grid unknown the members may have `Array` unknowns (constants the residuals multiply
    stencil terms by; any number, shape and position in the state, the same for all members).  Their state is packed
    beside the level-major grid state: x, m, v and g are then `_Levels` whose `.params` is a [B, P] tensor (P: the elements
    of all Arrays in state order); member b's kernels read its constants from its row (`a.par`), reduce their gradients
    over the grid into its rows of packed partial sums and of `pgrad` [B, npg] (the bodies of k_fwd / k_final / k_loss of
    the single run), and
      6. `ops.adam_step_params_batch`: ONE launch that forms g.params from `pgrad` through `param_rows` and updates
         x.params, m.params, v.params of all members -- behind the gathers, which re-read the constants.
    `levels(packed, b)` gives member b's arrays in `arrays_from_state` order, `blocks(packed)` the [B, size] views an
    optimizer on member-major vectors works with, `total` counts the parameters.  Members without `Array` unknowns make
    exactly the launches 1 - 5.

    `NeuralNet` unknowns (pointwise networks the residuals evaluate, `ctx.neural_net(key)`) are packed the same way: every
    array of a network is a ("param", offset, shape) item of `order`, weights then biases as `arrays_from_state` has them,
    its gradient rows are those of `pg_decl` (all `pw` groups layer by layer, then all `pb` groups; a weight matrix is
    stored (no, ni), row j * ni + i its contiguous element), -1 in `param_rows` where no grid kernel writes one (a network
    read only with frozen=True, an Array that appears only in a prior).  The operators are generated with batch="params".

    Outputs in parameter space (a weight decay, heat's `wreg`, a prior on an Array: `TracedOperator.par_outputs`) run as
      6a. `k_par_batch` (`EpochBatch.launch_par`), one launch per group, behind k_loss_batch: member b's terms and norms
          into its row of the group's `pout`, the term added to its loss, its gradients added to its row of `gextra`
          [B, P], which is zero before -- SET where no grid kernel writes (the `fresh` rule of `param_expr.emit`);
      6b. launch 6 with `extra=gextra` (odil_adam_step_params_extra_batch): g.params = pgrad[row] + gextra, the update,
          and gextra cleared for the next epoch
    -- the sums of a single run (pgrad -> gviews, k_par adds, one Adam step over the packed vector), whose bits every
    member keeps, in ONE parameter launch beside `k_par_batch`; members without such outputs keep launch 6 as it was.
    `report` inserts the parameter-space terms and norms at their outputs' positions.
    SEVERAL grid unknowns, node-centred axes: the F grid unknowns of a member share one location string (any mix of 'c'
    and 'n'), one kind and their level shapes, and are STACKED on the member axis: x, m, v, g (and u) hold one
    [F B, *shape] tensor per level, row f B + b for field f (`grid_keys` order) of member b; `loc` is "." + that location.
    Launch 1 then synthesises all fields of all members, launch 4 is `ops.mg_synth_adj_adam_members` -- ONE chain for all
    rows, the fast / marching kernel where a single member's level runs it, `k_interp_adj_members` where a single member
    runs the generic transpose (a node-centred y or x axis) -- and launch 5 updates level 0 of all rows; the step sizes
    of the rows are prepared once per run (`step_rows`).  `order` items are ("level", l, f); `levels`, `blocks`, `ranges`
    and `total` follow `arrays_from_state`: field by field, level by level, parameters where the state has them.  ONE
    cell-centred unknown (`stacked` False) makes exactly the launches 1 - 5 above.
    4-D members (velocity_from_tracer/veltracer3d: u, vx, vy, vz at 'nccc' on (t, x, y, z)) always take the stacked rows,
    even ONE 'cccc' unknown (`stacked` True): "." + loc would have five axes, one more than the transfer kernels know, so
    launch 1 is `ops.mg_synth_members` and launch 4 runs the row variants of the three transposes a single 4-D array
    takes (generic, fast, 'nccc' marching), the row on a grid dimension the single kernel leaves free.
    Not served: marching kernels, parameter-space outputs that only the torch replay evaluates."""

    def __init__(self, problems, states, form="launches"):
        """The members have passed the structural checks of `ensemble.optimize_ensemble` (the same grid unknowns, the same
        `Array` and `NeuralNet` unknowns, same level shapes, dtype and device; `traced_refusal` admits the shapes).  A member whose
        operator has no batched kernels raises ValueError naming it."""
        from . import stencil_jit
        from .core import Array, NeuralNet
        from .stencil_bind import EpochBatch, field_ranges

        domain = problems[0].domain
        arrays = domain.arrays_from_state(states[0])
        # the state's arrays in `arrays_from_state` order: ("level", l) of the grid unknown, ("param", offset, shape) of
        # an `Array`, or of one array of a `NeuralNet` (weights, then biases), in the members' packed parameters
        self.order, self.param_keys, self.nparams, self.ranges, self.grid_keys = [], [], 0, [], []
        for key, field, pos, n in field_ranges(domain, states[0]):
            kind = "net" if isinstance(field, NeuralNet) else "array" if isinstance(field, Array) else "grid"
            self.ranges.append((key, kind, pos, n))
            if isinstance(field, (Array, NeuralNet)):
                start = self.nparams
                for a in arrays[pos:pos + n]:
                    shape = tuple(int(k) for k in a.shape)
                    self.order.append(("param", self.nparams, shape))
                    self.nparams += math.prod(shape)
                self.param_keys.append((key, start, self.nparams - start))
            else:  # (grid unknown number f: its levels are the rows f B ... f B + B - 1 of the level tensors)
                if not self.grid_keys:
                    first, nlvl, loc = pos, n, field.loc
                self.order.extend(("level", l, len(self.grid_keys)) for l in range(n))
                self.grid_keys.append(key)
        shapes = [tuple(int(n) for n in a.shape) for a in arrays[first:first + nlvl]]
        dtype, device = arrays[first].dtype, arrays[first].device
        nb, nfields = len(problems), len(self.grid_keys)
        reason = traced_refusal(shapes, dtype, form, nb, loc=loc, nfields=nfields)
        if reason is not None:
            raise ValueError("ensemble of {} members: {}".format(nb, reason))
        # one cell-centred unknown: the rules of the Poisson forms admitted it; else those of the stacked rows of any loc
        self.stacked = rows_stacked(nfields, loc)
        self.form = form
        self.traced = []
        for b, (problem, state) in enumerate(zip(problems, states)):
            try:
                self.traced.append(stencil_jit.TracedOperator(problem, state, batch="params"))
            except stencil_jit.TraceUnsupported as e:
                raise ValueError("ensemble member {}: its operator has no batched kernels ({})".format(b, e))
        self._allocate(shapes, dtype, device, [list(t.names) for t in self.traced], loc=loc, nfields=nfields)
        self.u = self.members(self.cshape) if self.nlvl > 1 else self.x[0]
        self.work = ([None] + [self.members(s) for s in self.shapes[1:-1]] + [None])[: self.nlvl]
        by_lib = dict()
        for b, traced in enumerate(self.traced):
            by_lib.setdefault(traced.lib_path, []).append(b)
        self.groups = list(by_lib.values())
        if self.param_keys:
            self._allocate_params()
        self.outs, self.batches, self.gextra = [], [], None
        for group in self.groups:
            out = torch.zeros((len(group), 1 + 2 * self.traced[group[0]].nout), dtype=self.dtype, device=self.device)
            self.outs.append(out)
            more, lead = dict(), self.traced[group[0]]
            if lead.cg.arrays or lead.cg.nets:
                more = dict(params=[self._member_params(b) for b in group], pgrad=[self.pgrad[b] for b in group])
            if lead.par_outputs:
                for i in lead.cg.par_index:
                    if self.order[i][0] != "param":
                        raise ValueError("ensemble member {}: an output in parameter space reads the grid unknown".format(group[0]))
                if self.gextra is None:  # (what k_par_batch leaves of the parameter gradients: `_param_step` adds it)
                    self.gextra = _Levels(self.g)
                    self.gextra.params = torch.zeros_like(self.g.params)
                more.update(par_vals=[[self.levels(self.x, b)[i] for i in lead.cg.par_index] for b in group],
                            par_grads=[[self.levels(self.gextra, b)[i] for i in lead.cg.par_index] for b in group])
            row = {key: f * nb for f, key in enumerate(self.grid_keys)}
            foreign = [key for key in lead.cg.src_keys if key not in row]
            if foreign:
                raise ValueError("ensemble member {}: its kernels read {} as grid arrays".format(group[0], foreign))
            self.batches.append(EpochBatch([self.traced[b] for b in group],
                                           [[self.u[row[key] + b] for key in lead.cg.src_keys] for b in group],
                                           [{key: self.g[0][at + b] for key, at in row.items()} for b in group], out, **more))
        self.where = dict((b, (k, j)) for k, group in enumerate(self.groups) for j, b in enumerate(group))
        self.index = [torch.tensor(group, device=self.device) for group in self.groups]
        if len(self.groups) == 1:  # (column 0 of the packed `out` itself: nothing to collect)
            self.loss = self.outs[0][:, 0]
        self.graphable = all(batch.graphable for batch in self.batches)
        self.par_batches = [batch for batch in self.batches if batch.npar_out]

    def _member_params(self, member):
        """{key: member b's view(s) of its row of x.params} as `EpochBatch` takes them: one array per `Array`, the list of
        its arrays (weights, then biases) per network."""
        levels, res = self.levels(self.x, member), dict()
        for key, kind, pos, n in self.ranges:
            if kind == "net":
                res[key] = levels[pos:pos + n]
            elif kind == "array":
                res[key] = levels[pos]
        return res

    def _allocate_params(self):
        """The packed state of the members' `Array` and `NeuralNet` unknowns beside the level-major grid state: x, m, v, g get `.params`,
        a [B, P] tensor each (P: the elements of all Arrays, in state order); `pgrad` [B, npg]: where member b's k_loss
        leaves the gradients of the rows of its `pg_decl`; `param_rows`: packed parameter -> its row there (-1: no grid
        kernel reads that Array with a gradient), one map [P] when all members' kernels agree, else a map per member."""
        self.total += self.nparams
        for name in "xmvg":
            levels = _Levels(getattr(self, name))
            levels.params = torch.zeros((self.nbatch, self.nparams), dtype=self.dtype, device=self.device)
            setattr(self, name, levels)
        rows = []
        for traced in self.traced:
            cg, row = traced.cg, []
            for key, _, n in self.param_keys:
                row.extend(range(cg.pg_offset[key], cg.pg_offset[key] + n) if key in cg.pgrads else [-1] * n)
            rows.append(row)
        npg = max(1, max(len(traced.cg.pg_decl) for traced in self.traced))
        self.pgrad = torch.zeros((self.nbatch, npg), dtype=self.dtype, device=self.device)
        self.param_rows = ops.param_rows(rows[0] if all(row == rows[0] for row in rows) else rows, npg, self.device)

    def levels(self, packed, member):
        """The arrays of one member in its `arrays_from_state` order: views of the [B, *shape] level tensors and, for
        `Array` unknowns, of its row of the packed parameters."""
        params, nb = getattr(packed, "params", None), self.nbatch
        return [packed[item[1]][item[2] * nb + member] if item[0] == "level"
                else params[member, item[1]:item[1] + math.prod(item[2])].view(item[2]) for item in self.order]

    def blocks(self, packed):
        params, nb = getattr(packed, "params", None), self.nbatch
        return [packed[item[1]][item[2] * nb:(item[2] + 1) * nb].view(nb, -1) if item[0] == "level"
                else params[:, item[1]:item[1] + math.prod(item[2])] for item in self.order]

    def step_rows(self, table):
        """The table of step sizes ([E] shared by all members, or [E, B]: a row per epoch) as the launches on the stacked
        rows read it: [E, nfields B], row f B + b with member b's step size -- prepared once for a run, not per epoch."""
        table = np.asarray(table)
        return np.tile(table, (1, self.nfields)) if table.ndim == 2 and self.nfields > 1 else table

    def _row_steps(self, alphas):
        """DEVICE step sizes of one epoch as the stacked rows read them: one element, or one per row (a [B] vector that
        `step_rows` has not prepared is repeated here)."""
        if self.nfields > 1 and alphas.numel() == self.nbatch and self.nbatch > 1:
            return alphas.repeat(self.nfields)
        return alphas

    def _synthesis(self):
        """Launch 1: u of all rows.  Rows of four axes have no '.' + loc view (it would have five axes):
        `ops.mg_synth_members` puts the row on a grid dimension."""
        if self.nlvl > 1 and self.ndim == 4:
            ops.mg_synth_members(self.x, self.loc[1:], work=self.work, out=self.u)
        elif self.nlvl > 1:
            ops.mg_synth(self.x, self.loc, work=self.work, out=self.u)

    def _param_step(self, alphas=None, omb1=0.0, omb2=0.0, eps=0.0):
        """ONE launch for the `Array` and `NeuralNet` unknowns of all members, behind the gathers (which re-read them): the
        packed parameter gradient from the rows k_loss_batch wrote -- plus what k_par_batch left in `gextra` -- and, with
        step sizes, the Adam update."""
        if not self.nparams:
            return
        extra = None if self.gextra is None else self.gextra.params
        if alphas is None:
            ops.adam_step_params_batch(None, None, None, self.g.params, self.pgrad, self.param_rows, extra=extra)
        else:
            ops.adam_step_params_batch(self.x.params, self.m.params, self.v.params, self.g.params, self.pgrad, self.param_rows,
                                       alphas, omb1, omb2, eps, extra=extra)

    def report(self, member, outs=None, pouts=None):
        """(loss, terms, norms) of `member` as the last epoch evaluated them: 0-d views of the packed `out` (outs, pouts: of
        copies of `self.outs` / `self.pouts` instead, which later epochs do not overwrite)."""
        k, j = self.where[member]
        row, nout = (outs or self.outs)[k][j], self.traced[member].nout
        terms, norms = [row[1 + i] for i in range(nout)], [row[1 + nout + i] for i in range(nout)]
        if self.traced[member].par_outputs:  # (at their outputs' positions, as `TracedOperator.eval_loss_grad` inserts them)
            pout = (pouts or self.pouts)[k][j]
            for q, (at, _) in enumerate(self.traced[member].par_outputs):
                terms.insert(at, pout[2 * q])
                norms.insert(at, pout[2 * q + 1])
        return row[0], terms, norms

    @property
    def pouts(self):
        """Per group the packed [B_k, 2 npar_out] terms and norms of its outputs in parameter space, None without any."""
        return [batch.pout for batch in self.batches]

    def _evaluate(self, alphas=None, omb1=0.0, omb2=0.0, eps=0.0):
        """Behind the gathers: the outputs in parameter space (k_par_batch adds their terms to the members' losses, which
        are collected after it), then the parameter gradients and, with step sizes, the update of the parameters."""
        if self.par_batches:
            for batch in self.par_batches:
                batch.launch_par()
            self._collect_loss()
        self._param_step(alphas, omb1, omb2, eps)

    def _collect_loss(self):
        """Column 0 of every group's `out` into `loss` [B] (one group: `loss` IS that column)."""
        if len(self.groups) > 1:
            for index, out in zip(self.index, self.outs):
                self.loss.index_copy_(0, index, out[:, 0])

    def epoch(self, alphas, omb1, omb2, eps):
        """One Adam epoch of every member; alphas: DEVICE step sizes, [B] or one element shared by all members.  The [B]
        losses the epoch evaluated (before its update) land in self.loss."""
        self._synthesis()
        for batch in self.batches:
            batch.launch()
        if not self.par_batches:
            self._collect_loss()
        rows = self._row_steps(alphas)
        if self.nlvl > 1:  # (all fields of all members: ONE chain)
            ops.mg_synth_adj_adam_members(self.g[0], self.shapes, self.loc[1:], self.g, self.x, self.m, self.v, rows, omb1, omb2,
                                          eps)
        ops.adam_step_batch(self.x[0], self.m[0], self.v[0], self.g[0], rows, omb1, omb2, eps)
        # (the parameters: one step size per MEMBER -- the leading B of the stacked rows')
        self._evaluate(rows[:self.nbatch] if rows.numel() > self.nbatch else rows, omb1, omb2, eps)

    def loss_grad(self):
        self._synthesis()
        for batch in self.batches:
            batch.launch()
        if not self.par_batches:
            self._collect_loss()
        self._transposes()
        self._evaluate()


def rows_stacked(nfields, loc):
    """Does `TracedLaunchEnsemble` run members with `nfields` grid unknowns at `loc` through the chain for stacked rows?
    Anything but ONE cell-centred unknown does, and every 4-D member: its rows have no '.' + loc view.  The transposed
    chain is the same either way; what this decides is whose rules admit the members (`traced_refusal`)."""
    return nfields > 1 or loc != "c" * len(loc) or len(loc) == 4


def traced_refusal(shapes, dtype, form, nbatch=1, loc=None, nfields=1):
    """Why members of these level shapes are not run by `TracedLaunchEnsemble` in `form` ('launches': 1-D / 2-D, 'volumes':
    three dimensions and more, i.e. 3-D and 4-D), or None: `launches_refusal` / `volumes_refusal`, the one-level case (a plain `Field`: no transfers) exempt from
    their two-level rule.  loc, nfields: the location string the members' grid unknowns share and how many a member has;
    anything but ONE cell-centred unknown runs the chain for stacked rows, and the library says whether every level of the
    nfields * nbatch rows would run what that level of one member runs (odil_mg_members_levels_ok).  A 4-D member always
    takes the stacked rows, even ONE 'cccc' unknown."""
    ndim = len(shapes[0])
    if ndim == 4:  # (always the stacked rows, even ONE 'cccc' unknown)
        loc = "c" * ndim if loc is None else loc
    if loc is not None and rows_stacked(nfields, loc):
        return _members_refusal(shapes, dtype, form, nbatch * nfields, loc)
    if not 1 <= ndim <= 3:
        return "{}-D grid: the batched launches of traced operators run 1-D to 4-D grids".format(ndim)
    if dtype not in (torch.float64, torch.float32):
        return "dtype {}: the kernels run float64 and float32".format(dtype)
    if (form == "volumes") != (ndim == 3):
        return "{}-D grid: form '{}' runs {} grids".format(ndim, form, "3-D" if form == "volumes" else "1-D and 2-D")
    if len(shapes) == 1:
        return None
    reason = (volumes_refusal if ndim == 3 else launches_refusal)(shapes, dtype)
    if reason is None and nbatch > 1:
        reason = _levels_refusal(shapes, nbatch, dtype)
    return reason


def _members_refusal(shapes, dtype, form, nrows, loc):
    """`traced_refusal` for members with several grid unknowns or node-centred axes (`nrows` stacked rows at `loc`)."""
    ndim = len(shapes[0])
    if not 1 <= ndim <= 4:
        return "{}-D grid: the batched launches of traced operators run 1-D to 4-D grids".format(ndim)
    if dtype not in (torch.float64, torch.float32):
        return "dtype {}: the kernels run float64 and float32".format(dtype)
    if (form == "volumes") != (ndim >= 3):
        return "{}-D grid: form '{}' runs {} grids".format(ndim, form, "3-D and 4-D" if form == "volumes" else "1-D and 2-D")
    reason = _unaligned_members(shapes, dtype)
    if reason is not None or len(shapes) == 1:
        return reason
    return _levels_refusal(shapes, nrows, dtype, loc)


def _levels_refusal(shapes, nrows, dtype=None, loc=None):
    """The library's answer (odil_mg_members_levels_ok), the question every form ends with: why a transfer level of `nrows`
    rows of these level shapes at `loc` (default: all axes cell-centred) would not compute what that level of one row
    computes (level count, extents, refinement, schedule limits, the kernel a level runs), or None."""
    from ._lib import i64, load

    lib = load()
    flat = [int(n) for shape in shapes for n in shape]
    ndim = len(shapes[0])
    # (a caller without a dtype, `launches_refusal(shapes)`, is answered for 8 bytes: the kind of a 1-D or 2-D level does
    # not depend on the element size, only the 3-D marching kernels choose by it)
    item = 4 if dtype == torch.float32 else 8
    if lib.odil_mg_members_levels_ok(i64(flat), len(shapes), ndim, (loc or "c" * ndim).encode(), int(nrows), item) == 0:
        return None
    return lib.odil_last_error().decode()


# The shape-only refusals that the forms share: each the reason, or None where it does not apply.  Every predicate below
# asks for those it needs, in its own order.
def _too_few_levels(shapes):
    if len(shapes) < 2:
        return "1 level: the batched launches need a multigrid field of at least 2 levels"


def _not_halving(shapes):
    if any(tuple(2 * n for n in b) != tuple(a) for a, b in zip(shapes, shapes[1:])):
        return "levels {} do not halve exactly".format([tuple(s) for s in shapes])


def _coarsest_too_small(shapes):
    if any(n < 2 for n in shapes[-1]):
        return "levels {}: every extent must be at least 2".format([tuple(s) for s in shapes])


def _unaligned_members(shapes, dtype):
    cells = math.prod(shapes[0])
    if dtype is not None and (cells * (8 if dtype == torch.float64 else 4)) % 16:
        return "a member of {} cells is not a multiple of 16 bytes (members lie back to back)".format(cells)


def volumes_refusal(shapes, dtype=None):
    """Why levels of these shapes are not run as batched launches of 3-D members (PoissonVolumeEnsemble), or None when
    they are.  From the shapes (and, for the alignment of the members and the transfer kernels, the dtype) alone; the
    limits of the kernels are the library's."""
    if len(shapes[0]) != 3:
        return "{}-D grid: the batched launches of volumes run 3-D grids".format(len(shapes[0]))
    reason = _too_few_levels(shapes) or _unaligned_members(shapes, dtype) or _not_halving(shapes)
    if reason is None and any(n < 4 for n in shapes[0]):
        reason = "levels {}: every extent of the finest level must be at least 4".format([tuple(s) for s in shapes])
    reason = reason or _coarsest_too_small(shapes)
    if reason is not None:
        return reason
    if dtype == torch.float32 and ops.adjoint_transpose_supported(shapes[0]):
        # a single run of this shape takes the one-pass adjoint + first transpose launch, which sums the transpose in
        # the LDS-tile kernel's order; the ensemble runs the separate kernels, and where the separate first transpose
        # is the row-marching kernel (float rows of 64 ... 256 cells) it rounds differently in the last bits
        from ._lib import i64, load

        if load().odil_interp_adj_kind(i64(shapes[1]), 3, b"ccc", 4) == 3:
            return ("levels {}: a float32 run of this shape takes the one-pass adjoint + transpose launch, and the "
                    "separate row-marching transpose of the ensemble rounds differently").format([tuple(s) for s in shapes])
    return _levels_refusal(shapes, 1, dtype)


def launches_refusal(shapes, dtype=None):
    """Why levels of these shapes are not run as batched launches (PoissonLaunchEnsemble), or None when they are.  From the
    shapes (and, for the alignment of the members, the dtype) alone; the limits of the kernels are the library's."""
    if len(shapes[0]) > 2:
        return ("{}-D grid: the batched launches run 1-D and 2-D grids (a 3-D run fuses the synthesis into its residual "
                "and the first transpose into its adjoint)".format(len(shapes[0])))
    return (_too_few_levels(shapes) or _not_halving(shapes) or _coarsest_too_small(shapes)
            or _unaligned_members(shapes, dtype) or _levels_refusal(shapes, 1, dtype))


def ensemble_form(form, shapes, dtype):
    """'workgroup', 'launches' or 'volumes': the form `util.optimize_ensemble(form=...)` runs members of these level
    shapes in.  A function of shapes and dtype alone; 'auto' takes 'volumes' for 3-D members, else the one-workgroup
    epochs when `small_refusal` admits the members."""
    if form not in ("workgroup", "launches", "volumes", "auto"):
        raise ValueError("optimize_ensemble: form '{}' is none of 'workgroup', 'launches', 'volumes', 'auto'".format(form))
    if form == "auto":
        if len(shapes[0]) == 3:
            return "volumes"
        return "workgroup" if small_refusal(shapes, dtype) is None else "launches"
    return form


def small_refusal(shapes, dtype, force=None, max_cells=None):
    """Why levels of these shapes are not run as whole epochs by one workgroup (odil_poisson_small_epochs), or None when
    they are: the predicate of `PoissonEvaluator.small_plan`.  (Asks the library, not a device: usable before any state
    exists.)  force / max_cells: `small_force` / `small_max_cells` of the evaluator, default the class's."""
    from ._lib import i64, load

    force = PoissonEvaluator.small_force if force is None else force
    max_cells = PoissonEvaluator.small_max_cells if max_cells is None else max_cells
    ndim, nlvl = len(shapes[0]), len(shapes)
    if not max_cells:
        return "the one-workgroup epochs are switched off (small_max_cells = 0)"
    if ndim > 2:
        return "{}-D grid: the one-workgroup epochs run 1-D and 2-D grids".format(ndim)
    if nlvl > 12:
        return "{} levels: the one-workgroup epochs take at most 12".format(nlvl)
    flat = [int(n) for shape in shapes for n in shape]
    resident = bool(load().odil_poisson_small_epochs_resident(i64(flat), nlvl, ndim, 8 if dtype == torch.float64 else 4))
    cells = math.prod(shapes[0])
    if not resident and not force and not (ndim == 1 and cells <= max_cells):
        return "{} cells are above the limit of the one-workgroup epochs (state resident in LDS, or 1-D up to {} cells)".format(
            cells, max_cells)
    return _not_halving(shapes)  # (as the kernel requires)


def newton_refusal(cshape, h2, dtype):
    """Why a Poisson problem of these cells and squared spacings is not a member of a Newton ensemble (one workgroup per
    member walks its whole multigrid hierarchy: gmg.EnsembleGMG, odil_stencil_solve_batch), or None when it is.  Host
    arithmetic only: usable before any state exists."""
    from .gmg import EnsembleGMG

    cshape = tuple(int(n) for n in cshape)
    ndim = len(cshape)
    if not 1 <= ndim <= 3:
        return "{}-D grid: the one-workgroup Newton solves run 1-D to 3-D grids".format(ndim)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    shapes, _, locs, _ = EnsembleGMG.plan(cshape, h2, npdt)
    if any(loc != "c" * ndim for loc in locs):
        return "cells too far from cubes: the hierarchy {} halves some axes only".format(shapes)
    cells = math.prod(cshape)
    if cells > EnsembleGMG.max_cells:
        return "{} cells are above the limit of the one-workgroup Newton solves ({})".format(cells, EnsembleGMG.max_cells)
    if len(shapes) > EnsembleGMG.max_levels:
        return "{} levels: the one-workgroup Newton solves take at most {}".format(len(shapes), EnsembleGMG.max_levels)
    if math.prod(shapes[-1]) > EnsembleGMG.max_coarsest:
        return "the coarsest level {} has {} unknowns, above the {} of the dense coarsest solve".format(
            shapes[-1], math.prod(shapes[-1]), EnsembleGMG.max_coarsest)
    return None


def newton_stencil_refusal(cshape, dtype):
    """Why a single-field (2 d + 1)-point operator on these cells is not a member of a Newton ensemble of
    variable-coefficient problems (gmg.EnsembleGMG.from_coeffs), or None -- as far as the shape alone tells: 1-D to 3-D,
    extents >= 4 (the limit of `gmg.recognise_stencil`), at most `EnsembleGMG.max_cells` cells, and a coarsest level that
    CAN come below `EnsembleGMG.max_coarsest` unknowns (every axis halved while it is even).  How many levels the
    coefficients ask for, and the coarsest level they stop at, `from_coeffs` reports.  Host arithmetic only."""
    from .gmg import EnsembleGMG

    cshape = tuple(int(n) for n in cshape)
    ndim = len(cshape)
    if not 1 <= ndim <= 3:
        return "{}-D grid: the one-workgroup Newton solves run 1-D to 3-D grids".format(ndim)
    if dtype not in (torch.float64, torch.float32):
        return "dtype {}: the kernels run float64 and float32".format(dtype)
    if any(n < 4 for n in cshape):
        return "extents {}: a stencil operator is recognised on 4 cells per axis or more".format(cshape)
    cells = math.prod(cshape)
    if cells > EnsembleGMG.max_cells:
        return "{} cells are above the limit of the one-workgroup Newton solves ({})".format(cells, EnsembleGMG.max_cells)
    least = list(cshape)
    for _ in range(EnsembleGMG.max_levels - 1):
        least = [n // 2 if n % 2 == 0 and n // 2 >= 2 else n for n in least]
    if math.prod(least) > EnsembleGMG.max_coarsest:
        return "the coarsest level {} has {} unknowns, above the {} of the dense coarsest solve".format(
            tuple(least), math.prod(least), EnsembleGMG.max_coarsest)
    return None


def newton_launches_refusal(cshape, dtype):
    """Why a single-field (2 d + 1)-point operator on these cells is not a member of a Newton ensemble run as batched
    launches (gmg.EnsembleLaunchGMG), or None -- as far as the shape alone tells: 1-D to 3-D, float64 / float32, extents
    >= 4 (the limit of `gmg.recognise_stencil`), at most `EnsembleLaunchGMG.max_member_cells` cells (the limit per member
    of the batched launches, below 2^31), and levels that CAN end in a one-workgroup tail (every axis halved while it is
    even): a level of at most `tail_max_cells` cells below the finest, from which at most `EnsembleGMG.max_levels` levels
    lead to at most `EnsembleGMG.max_coarsest` unknowns.  Which levels the coefficients ask for, `from_coeffs` reports.
    Host arithmetic only."""
    from .gmg import EnsembleLaunchGMG

    cshape = tuple(int(n) for n in cshape)
    ndim = len(cshape)
    if not 1 <= ndim <= 3:
        return "{}-D grid: the batched Newton solves run 1-D to 3-D grids".format(ndim)
    if dtype not in (torch.float64, torch.float32):
        return "dtype {}: the kernels run float64 and float32".format(dtype)
    if any(n < 4 for n in cshape):
        return "extents {}: a stencil operator is recognised on 4 cells per axis or more".format(cshape)
    cells = math.prod(cshape)
    if cells > EnsembleLaunchGMG.max_member_cells:
        return "{} cells are above the limit per member of the batched Newton solves ({})".format(
            cells, EnsembleLaunchGMG.max_member_cells)
    shapes = [cshape]
    while EnsembleLaunchGMG._tail_room(shapes, EnsembleLaunchGMG.tail_max_cells) and any(
            n % 2 == 0 and n // 2 >= 2 for n in shapes[-1]):
        shapes.append(tuple(n // 2 if n % 2 == 0 and n // 2 >= 2 else n for n in shapes[-1]))
    try:
        EnsembleLaunchGMG.split(shapes)
    except ValueError as e:
        return str(e).split(": ", 1)[1]
    return None


def _close(a, b, rtol):
    scale = max(float(b.abs().max()), 1e-300)
    return float((a - b).abs().max()) <= rtol * scale


def detect(problem, state):
    """Returns a fused evaluator for `problem`, or None to keep the generic path."""
    from .core import Field, MultigridField, State

    domain = problem.domain
    if len(state.fields) != 1:
        return None
    (key, field), = state.fields.items()
    ndim = domain.ndim
    if ndim > 3 or field.loc != "c" * ndim:
        return None
    if isinstance(field, MultigridField):
        if field.factors is not None and any(float(f) != 1.0 for f in field.factors):
            return None
        axes = field.axes or domain.mg_axes
        if axes is not None and not all(axes):
            return None
        shapes = [tuple(t.array.shape) for t in field.terms]
    elif isinstance(field, Field):
        shapes = [tuple(field.array.shape)]
    else:
        return None
    cshape = tuple(domain.cshape)
    if shapes[0] != cshape or any(s < 2 for s in cshape):
        return None
    dtype = shapes and (field.terms[0].array if isinstance(field, MultigridField) else field.array).dtype
    device = domain.mod.device
    npdt = np.float64 if dtype == torch.float64 else np.float32
    h2 = [npdt(domain.step_by_dim(i)) ** 2 for i in range(ndim)]
    rtol = 1e-11 if dtype == torch.float64 else 1e-4

    gen = torch.Generator(device="cpu").manual_seed(12345)
    probes = []
    for k in range(2):
        # probe A is the zero state: Lap(0) == 0 exactly, so rhs_eff = -f(0) carries no rounding
        if k == 0:
            u = torch.zeros(cshape, dtype=dtype, device=device)
        else:
            u = torch.randn(cshape, generator=gen, dtype=torch.float64).to(dtype).to(device)
        pstate = State(fields={key: Field(u, loc=field.loc, cshape=cshape)}, initialized=True)
        try:
            accessed = [False]
            values, grads, names = _probe(problem, pstate, accessed)
        except Exception:
            return None
        if accessed[0] or len(values) != 1 or tuple(values[0].shape) != cshape:
            return None
        probes.append((u, values[0], grads[0], names))
    (ua, fa, ga, names), (ub, fb, gb, _) = probes
    want = [(0,) * ndim]
    for i in range(ndim):
        want += [tuple(-1 if j == i else 0 for j in range(ndim)), tuple(1 if j == i else 0 for j in range(ndim))]
    if any(k[0] != key or k[2] != field.loc for k in ga):
        return None
    if sorted(k[1] for k in ga) != sorted(want):
        return None
    coeffs = ops.poisson_jac_coeffs(cshape, h2, dtype, device)
    for slot, shift in enumerate(want):
        a, b = ga.get((key, shift, field.loc)), gb.get((key, shift, field.loc))
        if a is None or b is None:
            return None
        if not _close(a, b, rtol) or not _close(a, coeffs[slot], rtol):
            return None
    rhs_eff = -fa  # ua == 0
    fb_fused, _ = ops.poisson_residual(ub, rhs_eff, h2)
    if not _close(fb_fused, fb, 1e-9 if dtype == torch.float64 else 1e-3):
        return None
    from .util import printlog

    try:
        printlog("odil_amd: operator recognised as zero-Dirichlet Poisson stencil -> fused HIP kernels")
    except Exception:
        pass
    return PoissonEvaluator(cshape, shapes, rhs_eff.contiguous(), h2, name=names[0], dtype=dtype, device=device)


def _probe(problem, pstate, accessed):
    """eval_operator_grad on a probe state, recording whether the operator read ctx.tracers."""
    from . import core

    domain = problem.domain
    arrays = domain.arrays_from_state(pstate)
    leaves = [a.detach().requires_grad_(True) for a in arrays]
    shadow = problem._shadow_state(pstate, leaves)
    with torch.enable_grad():
        ctx = core.Context(domain, shadow, extra=problem.extra, tracers=problem.tracers, distinct_shift=True)
        names, values = problem._split_outputs(problem.operator(ctx))
        accessed[0] = ctx.tracers_accessed or bool(ctx.key_to_array_jac)
        if any(isinstance(v, core.Context.Raw) for v in values):
            accessed[0] = True
            return [], [], names
        grads = []
        for v in values:
            descs = list(ctx.desc_to_array.keys())
            symbols = [ctx.desc_to_array[d] for d in descs]
            gg = torch.autograd.grad(v.sum(), symbols, allow_unused=True, retain_graph=True)
            grads.append(dict(zip(descs, gg)))
    return [v.detach() for v in values], grads, names
