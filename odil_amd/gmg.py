"""Geometric multigrid for the Newton step of Poisson-type operators on the device.

The reference solves the Newton system through the normal equations with SuperLU
(`linsolver.solve(..., "direct")`, reference src/odil/linsolver.py:17-26) or, with
`--linsolver multigrid`, pyamg's smoothed aggregation + CG (linsolver.py:61-72).  Neither
scales to the 1.3e8 unknowns of the 512^3 configuration.  When the linearised operator is the
(square, nonsingular) zero-Dirichlet Laplacian stencil -- recognised from its coefficient
arrays, as in fused.py -- `M^T M d = -M^T r` and `M d = -r` have the same solution, and the
latter is solved here by V-cycles built only from the HIP kernels of the hot path:

  smoother      damped Jacobi: x' = x - omega (A x - b) / diag    odil_poisson_jacobi (one pass, 3 words per cell)
  restriction   cell-centred full weighting (mean of 2^d cells)    odil_restrict
  prolongation  x += P(x_c), the multigrid-decomposition P         odil_interp_add
  coarse grids  the same stencil re-discretised with h_l = 2^l h   odil_poisson_jac_coeffs (diag)

Convergence is checked on the true residual with the deterministic dot products.
"""

import collections
import math

import ctypes

import numpy as np
import torch

from . import ops

ctypes_int = ctypes.c_int


def skewed(shape, dtype, device, k, zero=False):
    """A work array whose base address is moved k x 4 KB off its allocation.  The arrays of a 512^3 float64 level are
    exactly 2^30 bytes each; allocated back to back they start 2^30 bytes apart, and the streams of a sweep (x, b, x') then
    walk the same memory channels in step: 0.66 against 0.61 ms for a sweep, 0.81 against 0.77 for a pair
    (tools/mb_alias.py: any offset from 256 B up removes it)."""
    n = math.prod(shape)
    pad = (k % 16) * 4096 // torch.empty((), dtype=dtype).element_size()
    flat = (torch.zeros if zero else torch.empty)(n + pad, dtype=dtype, device=device)
    return flat[pad:pad + n].view(shape)


def jacobi_weights(ndim, n):
    """The weights of n Jacobi sweeps that form the degree-n Chebyshev polynomial on [1 / ndim, 2], the part of the
    spectrum of D^-1 A that the coarse grid cannot see (`PoissonGMG.smooth`)."""
    return chebyshev_weights(n, 1.0 / ndim, 2.0)


def poisson_hierarchy(shape, h2, npdt, min_size=2):
    """(shapes, h2s, locs) of the rediscretised Poisson hierarchy below `shape` (host arithmetic only; the rule is
    described in `PoissonGMG.__init__`)."""
    shapes, h2s, locs = [tuple(shape)], [[npdt(v) for v in h2]], []
    while True:
        cur, h = shapes[-1], h2s[-1]
        hmin = min(float(v) for v in h)
        halve = [float(v) <= 2.0 * hmin for v in h]
        if not all(n % 2 == 0 and n // 2 >= min_size for n, on in zip(cur, halve) if on):
            break
        shapes.append(tuple(n // 2 if on else n for n, on in zip(cur, halve)))
        h2s.append([v * npdt(4) if on else v for v, on in zip(h, halve)])
        locs.append("".join("c" if on else "." for on in halve))
    return shapes, h2s, locs


class PoissonGMG:
    nu_default = (2, 2)  # pre- / post-smoothing sweeps of a cycle

    def __init__(self, shape, h2, dtype, device, omega=None, nu1=None, nu2=None, min_size=2, lite=False):
        """lite: the finest level's operator only, no work arrays of the cycle -- the float64 half of a mixed-precision
        solve (`solve_mixed`), which needs this object for the residual alone."""
        self.ndim = len(shape)
        self.loc = "c" * self.ndim
        self.dtype, self.device = dtype, device
        npdt = np.float64 if dtype == torch.float64 else np.float32
        # SEMI-coarsening while the cells are far from cubes: point smoothing only damps what oscillates along the strongly
        # coupled axes (the small spacings), so only those are halved -- the axes whose h^2 is within a factor 2 of the
        # smallest -- until the spacings meet; from there on (and from the start on a grid of cubes) every axis is halved.
        # 1024 x 64 on the unit square: (512, 64), (256, 64), (128, 64), (64, 64), (32, 32), ...  With full coarsening the
        # cycles lost their rate at cells 1 : 2 (24 passes with the Krylov hand-over), 1 : 4 (70 - 110) and failed at 1 : 16.
        # locs: per transition lvl -> lvl + 1: 'c' on the halved axes, '.' on the others
        self.shapes, self.h2s, self.locs = poisson_hierarchy(shape, h2, npdt, min_size)
        self.finish_init(omega, nu1, nu2, lite)

    def finish_init(self, omega, nu1, nu2, lite):
        """What a hierarchy of either operator needs once `shapes` stands: the cycle's parameters, caches, work arrays."""
        dtype, device = self.dtype, self.device
        self.omega = omega if omega is not None else {1: 2.0 / 3.0, 2: 4.0 / 5.0, 3: 6.0 / 7.0}[self.ndim]
        self.nu1 = self.nu_default[0] if nu1 is None else nu1
        self.nu2 = self.nu_default[1] if nu2 is None else nu2
        self.nlvl = len(self.shapes)
        self.loss = torch.zeros((), dtype=dtype, device=device)
        self._coarse_inv = None
        self._continuation = None
        self._r = [None] * self.nlvl                         # residuals (only where the fused restriction cannot be used)
        if lite:
            return
        self.x = [None] + [skewed(s, dtype, device, 2, zero=True) for s in self.shapes[1:]]   # coarse corrections
        self.b = [None] + [skewed(s, dtype, device, 3, zero=True) for s in self.shapes[1:]]   # coarse right-hand sides
        self.spare = [skewed(s, dtype, device, 1) for s in self.shapes]  # target of a sweep / prolongation

    residual_sign = 1.0  # `residual` returns A x - b

    def coarse_inverse(self):
        """Inverse of the coarsest-grid operator (at most a few dozen unknowns), built once from the
        residual kernel applied to unit vectors: the coarsest solve is then one product (odil_dots)
        instead of dozens of launch-bound sweeps."""
        if self._coarse_inv is None:
            shape = self.shapes[-1]
            n = math.prod(shape)
            eye = torch.eye(n, dtype=self.dtype, device=self.device)
            zero = torch.zeros(shape, dtype=self.dtype, device=self.device)
            cols = [self.coarse_column(eye[j].view(shape), zero).reshape(-1) for j in range(n)]
            amat = torch.stack(cols, dim=1).cpu().numpy().astype(np.float64)  # column j = A e_j
            self._coarse_inv = torch.as_tensor(self.invert(amat), dtype=self.dtype).to(self.device).contiguous()
        return self._coarse_inv

    def coarse_column(self, e, zero):
        """A e on the coarsest level."""
        return ops.poisson_residual(e, zero, self.h2s[-1])[0]

    invert = staticmethod(np.linalg.inv)

    def r(self, lvl):
        if self._r[lvl] is None:
            self._r[lvl] = torch.empty(self.shapes[lvl], dtype=self.dtype, device=self.device)
        return self._r[lvl]

    def residual(self, lvl, x, b, out):
        """out = A x - b."""
        ops.poisson_residual(x, b, self.h2s[lvl], fu=out, loss=self.loss)
        return out

    def smooth(self, lvl, x, b, n, chebyshev=True, zero=False):
        """n Jacobi sweeps, each ONE kernel (odil_poisson_jacobi: x' = x - omega_k (A x - b) / diag); the
        iterate ping-pongs between `x` and the level's spare buffer.  Returns the tensor holding it.
        The weights omega_k are those of the degree-n Chebyshev polynomial on [1/d, 2], the part of the
        spectrum of D^-1 A that the coarse grid cannot see (eigenvalues (1/d) sum_i (1 - cos theta_i) with
        some |theta_i| >= pi/2): two sweeps damp it by 0.34 (d = 3) where omega = 6/7 gives 0.51, three by
        0.15 instead of 0.36.  zero: the iterate is the zero vector and `x` only a buffer -- its content is not read."""
        return self.sweeps(lvl, x, b, self.weights(n, chebyshev), zero=zero)

    def weights(self, n, chebyshev=True):
        return jacobi_weights(self.ndim, n) if chebyshev else [self.omega] * n

    def sweeps(self, lvl, x, b, weights, zero=False):
        """Sweeps with the given weights, in PAIRS through the one-pass kernel (`sweep_pair`; bit-identical to two single
        sweeps) on levels large enough to be bandwidth-bound.  zero: the iterate is the zero vector (every coarse level of
        a cycle starts there) and `x` only a buffer: the first launch does not read it (x = NULL) -- the same bits as from
        an array of zeros, which nobody has to write."""
        weights = list(weights)
        if zero and (not weights or not self.zero_start):
            x.zero_()
            zero = False
        pair = self.pair_eligible(lvl)
        while weights:
            y = self.spare[lvl]
            src = None if zero else x
            zero = False
            if pair and len(weights) >= 2:
                self.sweep_pair(lvl, src, b, weights[0], weights[1], y)
                weights = weights[2:]
            else:
                self.sweep(lvl, src, b, weights[0], y)
                weights = weights[1:]
            self.spare[lvl] = x
            x = y
        return x

    def sweep(self, lvl, src, b, w, out):
        ops.poisson_jacobi(src, b, self.h2s[lvl], w, out=out)

    def sweep_pair(self, lvl, src, b, w1, w2, out):
        """(odil_poisson_jacobi2: the intermediate iterate stays on the CU, 3 words per cell and pair instead of 6)"""
        ops.poisson_jacobi2(src, b, self.h2s[lvl], w1, w2, out=out)

    def pair_eligible(self, lvl):
        # (float64 only: with four floats per lane the pair is bound by the vector ALU, 0.85 against 0.70 ms at 512^3)
        return (self.dtype == torch.float64 and ops.jacobi2_supported(self.shapes[lvl], self.dtype)
                and math.prod(self.shapes[lvl]) >= self.pair_min_cells)

    post_pair = True
    zero_start = True  # (False: the zero iterate of a coarse level is written and read back -- the tests compare both, bit for bit)
    pair_min_cells = 128**3  # below: the levels are launch-bound and the single-sweep kernels' smaller workgroups fill the chip better (measured: 128^3 / 64^3 / 32^3 as the threshold -> 25.0 / 25.7 / 26.6 ms for the 256^3 diffusion step)

    # ---- the coarse tail in one launch --------------------------------------------------------------------------------
    tail_max_cells = 8192  # levels of at most this many cells form the tail (odil_stencil_vcycle_tail); 0: off

    def tail_coeffs(self, lvl):
        """Coefficient arrays [(2 d + 1), *shape] of level `lvl` (what the one-launch tail works on)."""
        return ops.poisson_jac_coeffs(self.shapes[lvl], self.h2s[lvl], self.dtype, self.device)

    def tail(self):
        """(first tail level, flat coefficient tensor, work tensor) when the hierarchy ends in levels small enough to be
        walked by ONE workgroup -- every level from the first with <= tail_max_cells cells (never the finest) down to a
        coarsest grid of <= 512 unknowns with its dense inverse --, else None."""
        key = (self.tail_max_cells, self.nu1, self.nu2)
        cached = self.__dict__.get("_tail")
        if cached is not None and cached[0] == key:
            return cached[1]
        res = None
        first = next((l for l in range(1, self.nlvl) if math.prod(self.shapes[l]) <= self.tail_max_cells), None)
        if first is not None:
            first = max(first, self.nlvl - 8)  # (at most eight levels per launch: long 1-D hierarchies enter it lower down)
        if (self.tail_max_cells and first is not None and math.prod(self.shapes[-1]) <= 512
                and self.nu1 <= 4 and self.nu2 <= 4 and self.tail_transfers_ok(first)):
            flat = torch.cat([self.tail_coeffs(l).reshape(-1) for l in range(first, self.nlvl)])
            work = torch.empty(3 * sum(math.prod(s) for s in self.shapes[first:]), dtype=self.dtype, device=self.device)
            outs = [torch.empty(self.shapes[first], dtype=self.dtype, device=self.device) for _ in range(2)]
            res = (first, flat, work, outs)
        self.__dict__["_tail"] = (key, res)
        return res

    def tail_transfers_ok(self, first):
        """(the rediscretised hierarchy restricts with P^T / 2^k on semi-coarsened transitions, the tail with the mean of the
        children: the same only where every axis is halved)"""
        return all(loc == self.loc for loc in self.locs[first:])

    def tail_cycle(self, lvl, x, b, fmg=False):
        """One V-cycle (fmg: the nested-iteration start) on level `lvl` = the first tail level, in one launch."""
        first, flat, work, outs = self.tail()
        # (two result buffers in turn: a result may be the start iterate of the next call -- the second cycle on the first
        # coarse level of the variable-coefficient hierarchy -- and is otherwise consumed before the call after the next)
        out = outs[0] if x is None or x.data_ptr() != outs[0].data_ptr() else outs[1]
        launch = self.__dict__.get("_tail_launch")
        if launch is None or launch.keep[0] is not flat:  # (the launch's constant arguments, prepared once)
            launch = self._tail_launch = ops.stencil_vcycle_tail_plan(
                flat, self.shapes[first:], [[c == "c" for c in loc] for loc in self.locs[first:]], work, self.coarse_inverse(),
                self.weights(self.nu1), self.weights(self.nu2))
        return launch(x, b, out, fmg)

    def coarse_rhs(self, lvl, x, b):
        """b_{lvl+1} = R (b - A x), and mean((A x - b)^2) in self.loss.  One fused pass in 3-D (the fine
        residual is never stored); residual, restriction and sign as three launches otherwise."""
        bc = self.b[lvl + 1]
        if self.locs[lvl] == self.loc and ops.residual_restrict_supported(self.shapes[lvl], self.dtype):
            # (the norm is the SOLVE's measure on the finest level; a coarser level's is nobody's: no reduction launch)
            ops.poisson_residual_restrict(x, b, self.h2s[lvl], -1.0 / 2**self.ndim, bc, self.loss if lvl == 0 else None)
        else:
            r = self.residual(lvl, x, b, self.r(lvl))
            self.restrict(lvl, r, -1.0, out=bc)
        return bc

    def restrict(self, lvl, r, sign=1.0, out=None):
        """sign * R r onto level lvl + 1.  Every axis halved: the mean of the children (`odil_restrict`).  Some axes only:
        the transposed interpolation scaled to unit row sums, P^T / 2^k (`odil_restrict` SUBSAMPLES a '.' axis, as the
        reference's strided convolution does, core.py:745-751: not a restriction along it)."""
        loc = self.locs[lvl]
        if loc == self.loc:
            rc = ops.restrict_to_coarser(r, loc)
            return rc if sign == 1.0 and out is None else ops.scale(rc, sign, out=out)
        return ops.scale(ops.interp_adj(r, loc, self.shapes[lvl + 1]), sign / 2 ** loc.count("c"), out=out)

    def finish_cycle(self, lvl, x, b, post=True):
        """Second half of a V(nu1, nu2) cycle: `x` is pre-smoothed and b_{lvl+1} holds its restricted
        residual.  Coarse-grid correction and post-smoothing (post=False: none -- the caller smooths next anyway);
        returns the tensor holding the new iterate."""
        xc_new = self.coarse_correction(lvl)
        out = self.spare[lvl]
        weights = self.weights(self.nu2) if post else []
        pair = self.post_pair and len(weights) >= 2 and self.pair_eligible(lvl)
        if pair:
            # x + P x_c as a pass of its own (2 1/8 words), then the post-smoothing PAIR in one pass (3 words): 5 1/8
            # against 3 1/8 + 3 for the prolongation fused into the first of two single sweeps
            ops.interp_add(xc_new, self.locs[lvl], add=x, out=out)
        elif weights and self.locs[lvl] == self.loc and ops.jacobi_synth_supported(self.shapes[lvl], self.dtype):
            # x + P x_c is formed in registers by the first post-smoothing sweep (3 1/8 words per cell instead of 5 1/8)
            ops.poisson_jacobi_synth(xc_new, x, b, self.h2s[lvl], weights[0], out=out)
            weights = weights[1:]
        else:
            ops.interp_add(xc_new, self.locs[lvl], add=x, out=out)  # x + P x_c
        self.spare[lvl] = x
        return self.sweeps(lvl, out, b, weights)

    def coarse_correction(self, lvl):
        """x_c with A_c x_c ~= b_{lvl+1}: one cycle on level lvl + 1 from the zero iterate."""
        xc = self.x[lvl + 1]
        t = self.tail()
        if t is not None and lvl + 1 == t[0]:
            return self.tail_cycle(lvl + 1, None, self.b[lvl + 1])  # (the zero start is not even stored)
        # (not zeroed: a cycle from the zero start does not read its iterate's buffer)
        xc_new = self.vcycle(lvl + 1, xc, self.b[lvl + 1], zero=True)
        if xc_new is not xc:  # keep the per-cycle buffer distinct from the level's spare
            self.x[lvl + 1] = xc_new
        return xc_new

    def last_level_coeffs(self):
        """The last level's operator as coefficient arrays [(2 d + 1), *shape] (what `continuation` pads)."""
        return ops.poisson_jac_coeffs(self.shapes[-1], self.h2s[-1], self.dtype, self.device)

    def continuation(self):
        """The hierarchy BELOW a last level that is too large for the dense inverse and cannot be halved because an extent
        is odd (N = 100: 100, 50, 25; N = 1000 in 2-D: ..., 125 x 125 = 15625 unknowns, where sweeps alone solve nothing and
        the cycles above stall): the same operator on the grid padded to even extents -- the added cells carry a small
        diagonal entry and no coupling in either direction, their unknowns and right-hand sides are zero -- as the finest
        level of a `StencilGMG` of its own (which continues the same way at its next odd level).  None when the level is
        small, even (extents below `min_size`), or couples across the padded end (a periodic axis)."""
        if self._continuation is None:
            shape = self.shapes[-1]
            child = False
            if math.prod(shape) > 512 and any(n % 2 for n in shape) and all(n >= 3 for n in shape):
                c = self.last_level_coeffs()
                inside = tuple(slice(0, n) for n in shape)
                closed = True
                for ax, n in enumerate(shape):
                    if n % 2:  # nothing may reach across the end that moves: -e at the first cell, +e at the last
                        lo = c[1 + 2 * ax].select(ax, 0)
                        hi = c[2 + 2 * ax].select(ax, n - 1)
                        closed = closed and float(lo.abs().max()) == 0.0 and float(hi.abs().max()) == 0.0
                if closed:
                    padded = tuple(n + n % 2 for n in shape)
                    cp = torch.zeros((c.shape[0],) + padded, dtype=c.dtype, device=c.device)
                    cp[0].fill_(1e-6 * (float(c[0].abs().mean()) or 1.0))
                    cp[(slice(None),) + inside] = c
                    child = (StencilGMG(cp, nu1=self.nu1, nu2=self.nu2), inside, padded)
            self._continuation = child
        return self._continuation or None

    def continued_cycle(self, x, b):
        """Two cycles of the padded hierarchy in place of the last level's solve."""
        child, inside, padded = self.continuation()
        lvl = self.nlvl - 1
        xp = torch.zeros(padded, dtype=self.dtype, device=self.device)
        bp = torch.zeros(padded, dtype=self.dtype, device=self.device)
        xp[inside] = x
        bp[inside] = b
        for _ in range(2):  # (one: the padded transition loses accuracy, 0.35 per cycle instead of 0.17 at 250^2 and 100^3)
            xp = child.vcycle(0, xp, bp)
        out = self.spare[lvl]
        out.copy_(xp[inside])
        self.spare[lvl] = x
        return out

    def vcycle(self, lvl, x, b, zero=False, post=True):
        """One V(nu1, nu2) cycle on A x = b; returns the tensor holding the new iterate.  zero: `x` is the zero vector."""
        t = self.tail()
        if t is not None and lvl == t[0]:
            return self.tail_cycle(lvl, None if zero else x, b)
        if lvl == self.nlvl - 1:
            if math.prod(self.shapes[lvl]) <= 512:  # coarsest grid: x = A^-1 b
                out = self.spare[lvl]
                ops.dots(self.coarse_inverse(), b.reshape(-1), out=out.view(-1))
                self.spare[lvl] = x
                return out
            if self.continuation() is not None:  # an odd extent: the cycle goes on below on the padded grid
                return self.continued_cycle(x.zero_() if zero else x, b)
            return self.smooth(lvl, x, b, 40, chebyshev=False, zero=zero)  # cannot coarsen further: by iteration
        x = self.smooth(lvl, x, b, self.nu1, zero=zero)
        self.coarse_rhs(lvl, x, b)
        return self.finish_cycle(lvl, x, b, post=post)

    def full_multigrid(self, b, post=True):
        """First iterate by nested iteration: the right-hand side is restricted to every level, the coarsest problem is
        solved, and each finer level starts one V-cycle from the prolongated solution of the level below.  Costs about
        one V-cycle of the finest level plus 1/7 and leaves the error near the discretisation level instead of O(1):
        the cycles that follow only have to cover the remaining distance to the tolerance."""
        t = self.tail()
        bottom = self.nlvl - 1 if t is None else t[0]  # (the tail restricts and nests on its own levels in one launch)
        fb = [b]
        for lvl in range(bottom):
            fb.append(self.restrict(lvl, fb[-1]))
        x = None
        for lvl in range(bottom, -1, -1):
            if x is None and t is not None:
                x = self.tail_cycle(lvl, None, fb[lvl], fmg=True)
                continue
            if x is None:
                start = skewed(self.shapes[lvl], self.dtype, self.device, 5, zero=True)
            else:
                # (a fresh tensor: the cycle's work buffers rotate underneath)
                start = ops.interp_add(x, self.locs[lvl], out=skewed(self.shapes[lvl], self.dtype, self.device, 5))
            # (the tensor returned is never this level's coarse-correction buffer self.x[lvl], which the next finer
            # cycle zeroes: a cycle rotates its argument with self.spare[lvl] only)
            # (post=False: the finest level's cycle ends at its coarse-grid correction -- `solve` pre-smooths right after,
            # and four sweeps in a row buy less than the pass they cost)
            x = self.vcycle(lvl, start, fb[lvl], post=post or lvl > 0)
        return x

    def solve_krylov(self, b, x, tol, maxiter, status=None, m=6):
        """A x = b by GCR(m) with one V-cycle (from the zero start) as the preconditioner, continuing from the iterate `x`:
        what the stationary cycles hand over to when they stop contracting well (cells far from cubes, convection-dominated
        rows).  Per pass: one cycle, one operator application, the Gram-Schmidt products of the new direction with the last
        m (one `odil_dots` + two `odil_lincomb` passes over the stored directions, coefficients on the device) and two
        updates; one read-back (the residual norm).  A need not be symmetric.  Returns (x, residual norm, passes)."""
        n = b.numel()
        dev, dt = b.device, b.dtype
        sign = self.residual_sign
        r = torch.empty_like(b)
        self.residual(0, x, b, r)                   # sign * (A x - b)
        ops.scale(r, -sign, out=r)                  # r = b - A x
        x = x.contiguous()
        Z = torch.empty((m, n), dtype=dt, device=dev)   # directions z_j and their images q_j = A z_j, q_j orthonormal
        Q = torch.empty((m, n), dtype=dt, device=dev)
        zero_b = torch.zeros_like(b)
        bn = float(ops.dots(b.view(1, -1), b.view(-1))[0]) ** 0.5
        res = float(ops.dots(r.view(1, -1), r.view(-1))[0]) ** 0.5
        it, have, e = 0, 0, None
        while it < maxiter and res > tol * max(bn, 1e-300) and res == res:
            if have == m:  # restart: the stored directions are dropped
                have = 0
            e = self.vcycle(0, torch.empty_like(b) if e is None else e, r, zero=True)   # M^-1 r (from the zero start)
            z, q = Z[have].view(b.shape), Q[have].view(b.shape)
            z.copy_(e)
            self.residual(0, z, zero_b, q)          # sign * A z
            if sign != 1.0:
                ops.scale(q, sign, out=q)
            if have:  # Gram-Schmidt against the stored images: ONE product launch, two combination launches
                nbeta = ops.scale(ops.dots(Q[:have], q.view(-1)), -1.0)
                ops.lincomb(q.view(-1), 1.0, Q[:have], nbeta)
                ops.lincomb(z.view(-1), 1.0, Z[:have], nbeta)
            inv = torch.rsqrt(ops.dots(q.view(1, -1), q.view(-1)))          # 1 / |q|, a one-element device tensor
            ops.scale(q, 1.0, adev=inv, out=q)
            ops.scale(z, 1.0, adev=inv, out=z)
            a = ops.dots(q.view(1, -1), r.view(-1))
            ops.lincomb(x.view(-1), 1.0, z.view(1, -1), a)
            ops.lincomb(r.view(-1), 1.0, q.view(1, -1), ops.scale(a, -1.0))
            have += 1
            it += 1
            res = float(ops.dots(r.view(1, -1), r.view(-1))[0]) ** 0.5
        return x, res, it

    def solve(self, b, tol=1e-12, maxiter=60, status=None, x0=None, copy=True, fmg=True, krylov="auto", b_meansq=None):
        """Solves A x = b to ||A x - b|| <= tol * ||b||.  The residual that is tested is the one every cycle
        forms anyway (after its pre-smoothing sweeps, on its way to the coarse grid): the iterate returned
        is that pre-smoothed one, so convergence costs no pass of its own.  b_meansq: 0-d device tensor holding mean(b^2)
        when the caller has it (the evaluation that produced b reduced it already): no pass over b for its norm."""
        n = b.numel()
        # a relative residual below ~50 ulp of the working precision cannot be reached: asking float32 for 1e-12 would
        # burn every cycle of `maxiter` and report nothing
        tol = max(tol, 50 * float(torch.finfo(self.dtype).eps))
        if x0 is not None:
            x = x0.clone()
        elif fmg and self.nlvl > 2:
            x = self.full_multigrid(b, post=False)
        else:
            x = torch.zeros_like(b)
        if b_meansq is not None:
            bn = math.sqrt(max(float(b_meansq), 0.0) * n)
        else:
            bn = float(ops.dots(b.view(1, -1), b.view(-1))[0]) ** 0.5
        res, it = bn, 0
        method = "gmg-vcycle"
        stagnated = False
        if self.nlvl == 1:
            # the finest level itself cannot be halved (an odd extent): its 'cycle' is the dense inverse (small), the padded
            # continuation, or sweeps -- as the preconditioner of GCR, which needs no contraction from it (the continuation
            # at the FINEST level contracts by 0.3 - 0.5 only, at 125^3 one mode even grows: the wall sits half a coarse
            # cell off on every padded level)
            x, res, it = self.solve_krylov(b, x, tol, maxiter, m=6)
            method = "GCR(6), preconditioner: " + ("padded multigrid cycles" if self.continuation() is not None else
                                                   "coarse inverse" if n <= 512 else "sweeps")
        while self.nlvl > 1:
            x = self.smooth(0, x, b, self.nu1)
            self.coarse_rhs(0, x, b)
            prev, res = res, math.sqrt(max(float(self.loss), 0.0) * n)
            if res <= tol * max(bn, 1e-300) or it >= maxiter:
                break
            slow = it >= 2 and (res >= 0.5 * prev or res != res)
            if slow and krylov != "never" and res > 1e3 * tol * max(bn, 1e-300) and res == res:
                # the cycles contract by less than 0.5 (or not at all) well above the tolerance: the same cycle becomes the
                # preconditioner of GCR (`solve_krylov`), which needs no contraction, only a useful direction per pass
                x = x.clone()  # (a buffer of its own: the cycle's work buffers rotate underneath)
                x, res, extra = self.solve_krylov(b, x, tol, maxiter - it, m=6)
                it += extra
                method = "gmg-vcycle + GCR(6)"
                break
            if it >= 3 and res >= 0.98 * prev:
                stagnated = res == res and res < bn  # at the rounding floor of the working precision (not: diverging)
                break
            x = self.finish_cycle(0, x, b)
            it += 1
        converged = res <= tol * max(bn, 1e-300)
        if not converged:
            from .util import printlog

            printlog("odil_amd: multigrid stopped at relative residual {:.2e} after {} cycles (tolerance {:.1e})".format(
                res / max(bn, 1e-300), it, tol))
        if status is not None:
            status["residual"] = res
            status["bnorm"] = bn  # (|b|: the caller that judges the residual against it need not reduce b again)
            status["niter"] = it
            status["method"] = method
            status["converged"] = converged
            # cycles that stopped gaining at the floor of the working precision (float32: cond * 6e-8 relative): nothing that
            # works in this precision gets further, least of all the normal equations
            status["stagnated"] = stagnated
        # the iterate may live in one of this object's work buffers: copy=False only for a caller that
        # consumes it before the next solve
        return x.clone() if copy else x


def solve_mixed(high, low, b, tol=1e-12, maxiter=60, status=None, fmg=True):
    """A x = b in float64 by ITERATIVE REFINEMENT around float32 V-cycles: every pass forms the float64 residual
    r = A x - b with `high` (one pass over the fine level, its norm on the way), hands -r / rms(r) in float32 to one cycle of
    `low` (the first pass: its nested-iteration start) and adds the correction back in float64 -- the cycle is a
    preconditioner, so its precision limits the contraction per pass (~0.17, far above float32 rounding), not the accuracy
    of the answer, which is the float64 residual's.  The cycle's traffic -- everything but one residual per pass -- is
    halved.  Conversions: `odil_narrow_scale` / `odil_widen_axpy`, the scale read from the device scalar the residual
    kernel wrote.  (No reference counterpart: the reference's direct solve is double throughout, linsolver.py:17-26; the
    Newton iterate it defines is reached to the same tolerance.)"""
    n = b.numel()
    tol = max(tol, 50 * float(torch.finfo(b.dtype).eps))
    x = torch.zeros_like(b)
    r = high.r(0)
    rl = torch.empty(b.shape, dtype=torch.float32, device=b.device)
    bn = float(ops.dots(b.view(1, -1), b.view(-1))[0]) ** 0.5
    res, it, e = bn, 0, None
    while True:
        high.residual(0, x, b, r)  # r = A x - b, high.loss = its mean square
        prev, res = res, math.sqrt(max(float(high.loss), 0.0) * n)
        if res <= tol * max(bn, 1e-300) or it >= maxiter or (it >= 3 and res >= 0.98 * prev):
            break
        ops.narrow_scale(r, rl, a=-high.residual_sign, msq=high.loss)  # right-hand side of the error equation A e = b - A x
        if it == 0 and fmg and low.nlvl > 2:
            e = low.full_multigrid(rl)
        else:
            e = low.vcycle(0, torch.empty_like(rl) if e is None else e, rl, zero=True)
        ops.widen_axpy(x, e, a=1.0, msq=high.loss)
        it += 1
    converged = res <= tol * max(bn, 1e-300)
    if not converged:
        from .util import printlog

        printlog("odil_amd: mixed-precision multigrid stopped at relative residual {:.2e} after {} passes (tolerance {:.1e})".format(
            res / max(bn, 1e-300), it, tol))
    if status is not None:
        status.update(residual=res, niter=it, method="gmg-vcycle (float32 cycles, float64 residual)", converged=converged)
    return x


class StencilGMG(PoissonGMG):
    """V-cycles for ANY (2 d + 1)-point operator with variable coefficients on a cell-centred grid (d <= 3): the Newton
    system M delta = -r of a single-field operator as `Problem.linearize` delivers it (reference core.py:1113-1217) --
    variable-coefficient diffusion, reaction and convection terms, any wall closure, periodic axes.  Same cycle as
    PoissonGMG (Chebyshev-weighted Jacobi sweeps, full-weighting restriction, the multigrid decomposition's P for the
    corrections, nested-iteration start); what differs is where the operators come from:

      fine level     the Jacobian's own coefficient arrays                    `coeffs` [(2 d + 1), *shape]
      coarse levels  odil_stencil_var_coarsen (csrc/stencil_mg.hip): aggregates of 2^d cells, piecewise-constant Galerkin
                     products of the second-order part (x 1/2), the antisymmetric part and the row sums -- formed once
                     per solve (the coefficients change with the state), 8/7 of one pass over the fine arrays
      sweeps         odil_stencil_var_smooth            (2 d + 1) + 3 words per cell (Poisson: 3)
      coarse rhs     odil_stencil_var_residual_restrict (2 d + 1) + 2 + 1 / 2^d words, the residual norm on the way

    M need not be symmetric; the cycle is a stationary iteration on M delta = -r itself (for a square nonsingular M the
    solution of the normal equations the reference forms, linsolver.py:17-23).  `solve` reports `converged`; the caller
    (linsolver.solve) falls back to the normal-equation routes when the cycles do not contract."""

    def __init__(self, coeffs, nu1=None, nu2=None, min_size=2, lite=False, store=None):
        """lite: the finest level only (the float64 half of `solve_mixed`); store: dtype the hierarchy is KEPT in (the
        coarse operators are formed in the precision of `coeffs` and cast level by level: the float32 half)."""
        shape = tuple(coeffs.shape[1:])
        self.ndim = len(shape)
        assert coeffs.shape[0] == 2 * self.ndim + 1 and self.ndim <= 3 and coeffs.is_contiguous()
        self.loc = "c" * self.ndim
        self.dtype, self.device = store or coeffs.dtype, coeffs.device
        self.coeffs, self.shapes = [coeffs], [shape]
        self.locs = []  # per transition: 'c' on the merged axes, '.' on the others
        cur = coeffs
        while not lite:
            # SEMI-coarsening while the couplings are of different sizes (cells far from cubes, anisotropic conductivities):
            # only the axes whose largest coupling is within a factor 2 of the largest of all are merged -- point smoothing
            # damps nothing else -- until they meet (one read-back per level, at set-up)
            if self.ndim == 1:
                halve = [True]
            else:
                size = ops.max_abs_rows(cur[1:]).cpu().numpy()  # (2 d arrays: two launches, one read-back)
                # (the smaller of the two directions: an upwind convection term inflates ONE of them, and it grows
                # relative to the diffusion on every coarser level -- that is not an anisotropy of the smoothing problem)
                strength = [min(float(size[2 * a]), float(size[2 * a + 1])) for a in range(self.ndim)]
                halve = [v >= 0.5 * max(strength) for v in strength]
            if not all(n % 2 == 0 and n // 2 >= min_size for n, on in zip(self.shapes[-1], halve) if on):
                break
            cur = ops.stencil_var_coarsen(cur, halve)
            self.coeffs.append(cur)
            self.shapes.append(tuple(n // 2 if on else n for n, on in zip(self.shapes[-1], halve)))
            self.locs.append("".join("c" if on else "." for on in halve))
        if store is not None and store != coeffs.dtype:
            assert coeffs.dtype == torch.float64 and store == torch.float32
            self.coeffs = [ops.narrow_scale(c.reshape(-1), torch.empty(c.numel(), dtype=store, device=c.device)).view(c.shape)
                           for c in self.coeffs]
        self.finish_init(None, nu1, nu2, lite)

    def coarse_column(self, e, zero):
        return -ops.stencil_var_residual(self.coeffs[-1], e, zero)

    @staticmethod
    def invert(amat):
        """The PSEUDO-inverse: a singular coarsest operator (all-periodic or all-Neumann problems: constants in the null
        space) gets the minimum-norm solution."""
        return np.linalg.pinv(amat, rcond=1e-12)

    residual_sign = -1.0  # `residual` returns b - A x (PoissonGMG: A x - b)

    def tail_coeffs(self, lvl):
        return self.coeffs[lvl]

    def tail_transfers_ok(self, first):
        return True  # (mean of the merged children on every transition: what the tail does)

    def last_level_coeffs(self):
        return self.coeffs[-1]

    def residual(self, lvl, x, b, out):
        """out = b - A x, its mean square in self.loss."""
        ops.stencil_var_residual(self.coeffs[lvl], x, b, out=out)
        ops.mean_reduce(out.reshape(-1), square=True, out=self.loss)
        return out

    def sweep(self, lvl, src, b, w, out):
        ops.stencil_var_smooth(self.coeffs[lvl], src, b, w, out=out)

    def sweep_pair(self, lvl, src, b, w1, w2, out):
        """(odil_stencil_var_smooth2: the coefficient arrays -- 7 of a sweep's 10 words in 3-D -- read once for both sweeps)"""
        ops.stencil_var_smooth2(self.coeffs[lvl], src, b, w1, w2, out=out)

    def pair_eligible(self, lvl):
        return ops.smooth2_supported(self.shapes[lvl]) and math.prod(self.shapes[lvl]) >= self.pair_min_cells

    def coarse_rhs(self, lvl, x, b):
        bc = self.b[lvl + 1]
        if self.locs[lvl] == self.loc:
            ops.stencil_var_residual_restrict(self.coeffs[lvl], x, b, 1.0 / 2**self.ndim, bc, self.loss if lvl == 0 else None)
        else:  # some axes only: the residual (its norm on the way), then the mean of the children
            self.restrict(lvl, self.residual(lvl, x, b, self.r(lvl)), 1.0, out=bc)
        return bc

    def restrict(self, lvl, r, sign=1.0, out=None):
        """sign * (mean of the children): the R of the aggregation-built coarse operators.  (P^T / 2^k, which the
        rediscretised Poisson hierarchy uses on its semi-coarsened transitions, is NOT consistent with them: across a
        1 : 1000 jump of the conductivity the cycle diverged.)  Merged axes only: a strided mean (torch), no kernel of
        this library averages along a subset of the axes."""
        loc = self.locs[lvl]
        if loc == self.loc:
            return PoissonGMG.restrict(self, lvl, r, sign, out)
        pairs, dims = [], []
        for n, l in zip(r.shape, loc):
            if l == "c":
                dims.append(len(pairs) + 1)
                pairs += [n // 2, 2]
            else:
                pairs.append(n)
        rc = r.reshape(pairs).mean(dim=dims)
        return ops.scale(rc, sign, out=out) if (sign != 1.0 or out is not None) else rc

    def finish_cycle(self, lvl, x, b, post=True):
        xc_new = self.coarse_correction(lvl)
        # TWO cycles on the first coarse level in 3-D (a W-cycle's top, V below): the aggregation-built coarse operators
        # are slightly less accurate than a rediscretisation at the walls, and a more exact level-1 solve takes the
        # contraction from 0.24 to 0.14 per cycle (17 -> 13 cycles to 1e-10, tests/test_stencil_gmg_host.py) for 1/7 more
        # work; a full W-cycle gains one more cycle and pays it back in ~700 launch-bound coarse launches
        if lvl == 0 and self.ndim == 3 and self.nlvl > 2:
            xc_new = self.vcycle(lvl + 1, xc_new, self.b[lvl + 1])
            self.x[lvl + 1] = xc_new
        out = self.spare[lvl]
        ops.interp_add(xc_new, self.locs[lvl], add=x, out=out)  # x + P x_c
        self.spare[lvl] = x
        return self.sweeps(lvl, out, b, self.weights(self.nu2) if post else [])


class EnsembleGMG:
    """B small systems of ONE shape solved side by side, every solve of all members in ONE launch with one workgroup per
    member (odil_stencil_solve_batch): residual, nested-iteration start, V-cycles down to the tolerance, the convergence
    decision and -- for a Newton step -- the update, without a host read-back in between.  Member b's iterate after k
    cycles is that of k launches of `ops.stencil_vcycle_tail` on its arrays alone, bit for bit.

    EnsembleGMG(shape, h2, dtype, device, nbatch): the constant-coefficient Poisson operator, shared by all members --
    levels, spacings, `poisson_jac_coeffs` and the coarsest inverse are those of the `PoissonGMG` hierarchy (min_size stops
    the coarsening earlier; by default where at most `max_levels` levels remain).
    EnsembleGMG([hierarchy, ...]): one hierarchy per member (`StencilGMG` objects of one shape, or anything with `shapes`,
    `locs`, `tail_coeffs`, `coarse_inverse`, `weights`, `nu1`, `nu2`): their operators and inverses are packed per member.
    EnsembleGMG.from_coeffs(coeffs [B, 2 d + 1, *shape]): the same per-member hierarchies, set up for all members at once
    in launches that do not grow with B; `rebuild` repeats the set-up in place (every Newton step of a nonlinear operator).

    However it was made, an object has these attributes (`core`; `solve`, `newton_step`, `status` and the drivers of
    ensemble.py rely on nothing else):
        nbatch, dtype, device, ndim, shapes, locs, halve, coeffs, inv, wpre, wpost, nu1, nu2, cells, work, method, krylov
    shapes: the levels, fine to coarse; halve / locs: per transition the axes that are halved, as booleans / as 'c' and
    '.'; coeffs: the operators of all levels, flat [ncoeff] when the members share them, else [B, ncoeff]; inv: the
    coarsest inverse [n, n] or [B, n, n]; wpre / wpost: the weights of the nu1 / nu2 sweeps before / after the coarse
    correction; cells: of the finest level; work: [B, need] scratch of the launch; method: what `status` reports.
    Only an object made by `from_coeffs` has `fine`, `level` and `rebuild` (ValueError on the others).

    krylov: "never" (the default) -- a member whose cycles stop contracting ends with converged=False or stagnated; "auto"
    -- such a member is handed to GCR(krylov_m) around the same cycle INSIDE the launch (odil_stencil_solve_krylov_batch,
    the hand-over rule of `PoissonGMG.solve`), still one launch and one read-back per solve; `work` grows by
    (2 krylov_m + 2) finest-level vectors per member.  A member that never meets the rule gets the bits of "never".
    `status` reports the cycle of the hand-over; `outcome` is [B, 3] then (passes, stop reason, hand-over cycle or -1)."""

    max_cells = 32768    # cells of a member's finest level (32^3, 128^2, 1-D up to 32768)
    max_levels = 8       # kTailMaxLev of csrc/vcycle_tail.hip
    max_coarsest = 512   # unknowns of the coarsest level (its dense inverse is applied by one workgroup)
    core = ("nbatch", "dtype", "device", "ndim", "shapes", "locs", "halve", "coeffs", "inv", "wpre", "wpost", "nu1", "nu2",
            "cells", "work", "method", "krylov")
    krylov, krylov_m = "never", 6  # (what an object has that was made without the keywords)

    @classmethod
    def plan(cls, shape, h2, npdt, min_size=None):
        """(shapes, h2s, locs, min_size) of the hierarchy a member of this shape gets: PoissonGMG's, cut after
        `max_levels` levels when it is longer (host arithmetic only)."""
        shapes, h2s, locs = poisson_hierarchy(shape, h2, npdt, 2 if min_size is None else min_size)
        if min_size is None:
            min_size = 2
            if len(shapes) > cls.max_levels:
                # (stops PoissonGMG at that level: no halved extent of it reaches min_size again)
                min_size = min(shapes[cls.max_levels - 1])
                shapes, h2s, locs = poisson_hierarchy(shape, h2, npdt, min_size)
        return shapes, h2s, locs, min_size

    def __init__(self, shape, h2=None, dtype=None, device=None, nbatch=None, min_size=None, nu1=None, nu2=None,
                 krylov="never", krylov_m=6):
        self._strength = None  # (the scratch of the set-up launches: only `from_coeffs` objects have one)
        self._set_krylov(krylov, krylov_m)
        if torch.is_tensor(shape):
            self.method = "gmg-vcycle (variable coefficients), one workgroup per member"
            self._init_coeffs(shape, nu1, nu2, 2 if min_size is None else min_size)
            return
        self.method = "gmg-vcycle, one workgroup per member"
        if isinstance(shape, (list, tuple)) and shape and not isinstance(shape[0], (int, np.integer)):
            members = list(shape)
            first = members[0]
            for b, h in enumerate(members):
                if [tuple(s) for s in h.shapes] != [tuple(s) for s in first.shapes] or list(h.locs) != list(first.locs) \
                        or h.dtype != first.dtype or (h.nu1, h.nu2) != (first.nu1, first.nu2):
                    raise ValueError("ensemble member {}: its hierarchy differs from member 0's".format(b))
            self.nbatch = len(members)
            coeffs = torch.stack([torch.cat([h.tail_coeffs(l).reshape(-1) for l in range(len(first.shapes))])
                                  for h in members]).contiguous()
            inv = torch.stack([h.coarse_inverse() for h in members]).contiguous()
        else:
            npdt = np.float64 if dtype == torch.float64 else np.float32
            min_size = self.plan(shape, h2, npdt, min_size)[3]
            first = PoissonGMG(shape, h2, dtype, device, min_size=min_size)
            self.nbatch = int(nbatch)
            coeffs = torch.cat([first.tail_coeffs(l).reshape(-1) for l in range(first.nlvl)])
            inv = first.coarse_inverse()
        self.dtype, self.device, self.ndim = first.dtype, first.device, len(first.shapes[0])
        self.nu1, self.nu2, self.wpre, self.wpost = first.nu1, first.nu2, first.weights(first.nu1), first.weights(first.nu2)
        self._finish([tuple(s) for s in first.shapes], [[c == "c" for c in loc] for loc in first.locs], coeffs, inv)

    def _set_krylov(self, krylov, krylov_m):
        if krylov not in ("never", "auto"):
            raise ValueError("EnsembleGMG: krylov '{}' is neither 'never' nor 'auto'".format(krylov))
        if not 1 <= int(krylov_m) <= 8:
            raise ValueError("EnsembleGMG: krylov_m = {} (1..8 directions)".format(krylov_m))
        self.krylov, self.krylov_m = krylov, int(krylov_m)

    @classmethod
    def from_coeffs(cls, coeffs, nu1=None, nu2=None, min_size=2, krylov="never", krylov_m=6):
        """One variable-coefficient operator per member, coeffs [B, 2 d + 1, *shape]: level by level what
        `StencilGMG(coeffs[b])` builds for every member -- coefficient arrays and coarsest pseudo-inverse bit for bit -- in
        launches whose number does not depend on B: per level ONE strength launch and one read-back of [B, 2 d] (the
        semi-coarsening decision of `StencilGMG.__init__`; none in 1-D), per transition ONE coarsen launch, then ONE launch
        for the dense coarsest matrices and one read-back; the pseudo-inverses are `StencilGMG.invert` per member on the
        host in float64.  The kernel walks one set of shapes: every member must take member 0's decision on every level,
        else ValueError (no object is made).  Coarsening stops under StencilGMG's rule or at `max_levels` levels."""
        return cls(coeffs, nu1=nu1, nu2=nu2, min_size=min_size, krylov=krylov, krylov_m=krylov_m)

    def _init_coeffs(self, coeffs, nu1, nu2, min_size):
        nb, ndim = int(coeffs.shape[0]), coeffs.dim() - 2
        if nb < 1 or not 1 <= ndim <= 3 or coeffs.shape[1] != 2 * ndim + 1:
            raise ValueError("EnsembleGMG.from_coeffs: coefficients {} are not [B, 2 d + 1, *shape] with d <= 3".format(
                tuple(coeffs.shape)))
        shape = tuple(int(n) for n in coeffs.shape[2:])
        self._check_fine(shape)
        self.nbatch, self.dtype, self.device, self.ndim = nb, coeffs.dtype, coeffs.device, ndim
        self.nu1 = PoissonGMG.nu_default[0] if nu1 is None else nu1
        self.nu2 = PoissonGMG.nu_default[1] if nu2 is None else nu2
        self.wpre, self.wpost = jacobi_weights(ndim, self.nu1), jacobi_weights(ndim, self.nu2)
        self._min_size, self._shape0 = min_size, shape
        self._strength = torch.empty((nb, 2 * ndim), dtype=self.dtype, device=self.device)
        self._plan(coeffs.reshape(nb, -1))

    def _check_fine(self, shape):
        """ValueError when members of this finest shape cannot be served (before anything is allocated)."""
        if math.prod(shape) > self.max_cells:
            raise ValueError("EnsembleGMG.from_coeffs: {} cells are above the limit of the one-workgroup solves ({})".format(
                math.prod(shape), self.max_cells))

    def _may_coarsen(self, shapes):
        """Whether a hierarchy that has the levels `shapes` so far may get one more."""
        return len(shapes) < self.max_levels

    def _pack(self, levels):
        """[B, ncoeff]: the levels [B, (2 d + 1) cells of the level] of every member, one after another."""
        return torch.cat(levels, dim=1).contiguous()

    def _work_elements(self, shapes):
        """Work elements per member of the launch that walks these levels; ValueError when one workgroup does not."""
        if self.krylov == "auto":
            need = ops.stencil_solve_krylov_batch_work(shapes, self.krylov_m)
        else:
            need = ops.stencil_solve_batch_work(shapes)
        if not need or len(shapes) > self.max_levels or math.prod(shapes[-1]) > self.max_coarsest:
            raise ValueError("EnsembleGMG: levels {} are not walked by one workgroup (at most {} levels, a coarsest level "
                             "of at most {} unknowns)".format(shapes, self.max_levels, self.max_coarsest))
        return need

    def _finish(self, shapes, halves, coeffs, inv):
        """The end of every construction (and of a `rebuild` that plans anew): the levels, their packed operators and
        coarsest inverses become the object's, with the work array and the launch plan that go with them; nothing is
        changed when one workgroup does not walk these levels."""
        need = self._work_elements(shapes)
        self.shapes, self.halve = shapes, halves
        self.locs = ["".join("c" if on else "." for on in halve) for halve in halves]
        self.coeffs, self.inv, self.cells = coeffs, inv, math.prod(shapes[0])
        self.work = torch.empty((self.nbatch, need), dtype=self.dtype, device=self.device)
        if self.krylov == "auto":
            self._launch = ops.stencil_solve_krylov_batch_plan(self.coeffs, self.shapes, self.halve, self.nbatch, self.work,
                                                               self.inv, self.wpre, self.wpost, self.krylov_m)
        else:
            self._launch = ops.stencil_solve_batch_plan(self.coeffs, self.shapes, self.halve, self.nbatch, self.work, self.inv,
                                                        self.wpre, self.wpost)
        self._out = dict()      # maxcycles -> (history, outcome) device tensors
        self.history = None     # [B, maxcycles + 2], [B, 2] ("auto": [B, 3]) of the last launch on the host
        self.outcome = None
        missing = [name for name in self.core if not hasattr(self, name)]
        assert not missing, "EnsembleGMG lacks {}".format(missing)

    def _decide(self, level, lvl, shape):
        """The `halve` of `StencilGMG.__init__` for the level `level` [B, (2 d + 1) cells] of every member (one launch, one
        read-back), or None where its coarsening stops; ValueError when a member decides otherwise than member 0."""
        if len(shape) == 1:
            halve = [True]
        else:
            size = ops.stencil_strength_batch(level, shape, out=self._strength).cpu().numpy().astype(np.float64)
            strength = np.minimum(size[:, 0::2], size[:, 1::2])
            every = strength >= 0.5 * strength.max(axis=1, keepdims=True)
            blocked = np.array([not (n % 2 == 0 and n // 2 >= self._min_size) for n in shape])
            if (every & blocked).any(axis=1).all():
                return None  # (every member's coarsening stops here, whichever axes it would merge)
            differ = np.nonzero((every != every[0]).any(axis=1))[0]
            if len(differ):
                b = int(differ[0])
                raise ValueError("EnsembleGMG: member {} merges the axes {} on level {}, member 0 the axes {}: the members of an "
                                 "ensemble walk one set of levels".format(b, [bool(v) for v in every[b]], lvl,
                                                                          [bool(v) for v in every[0]]))
            halve = [bool(v) for v in every[0]]
            if not any(halve):
                raise ValueError("EnsembleGMG: the couplings of level {} are not finite".format(lvl))
        if not all(n % 2 == 0 and n // 2 >= self._min_size for n, on in zip(shape, halve) if on):
            return None
        return halve

    def _plan(self, fine):
        """Builds shapes, the packed hierarchy [B, ncoeff] and the inverses from the finest coefficients
        [B, (2 d + 1) cells]; the object is changed only once everything stands."""
        shapes, halves, levels = [self._shape0], [], [fine]
        while self._may_coarsen(shapes):
            halve = self._decide(levels[-1], len(shapes) - 1, shapes[-1])
            if halve is None:
                break
            levels.append(ops.stencil_var_coarsen_batch(levels[-1], shapes[-1], halve))
            shapes.append(tuple(n // 2 if on else n for n, on in zip(shapes[-1], halve)))
            halves.append(halve)
        self._work_elements(shapes)  # (before the dense matrices of a coarsest level that is too large are formed)
        ninv = math.prod(shapes[-1])
        coeffs = self._pack(levels)
        dense = torch.empty((self.nbatch, ninv, ninv), dtype=self.dtype, device=self.device)
        inv = torch.empty_like(dense)
        self._invert(levels[-1], shapes[-1], dense, inv)
        self._finish(shapes, halves, coeffs, inv)
        self._dense = dense
        sizes = [(2 * self.ndim + 1) * math.prod(s) for s in shapes]
        self._offsets = [sum(sizes[:l]) for l in range(len(sizes) + 1)]

    def _invert(self, coarsest, shape, dense, inv):
        """inv[b] = StencilGMG.invert(the dense matrix of member b's coarsest operator): one launch, one read-back, the
        pseudo-inverses on the host in float64, one copy back."""
        amat = ops.stencil_dense_batch(coarsest, shape, out=dense).cpu().numpy().astype(np.float64)
        host = np.stack([StencilGMG.invert(amat[b]) for b in range(self.nbatch)])
        inv.copy_(torch.as_tensor(host, dtype=self.dtype))

    def level(self, lvl):
        """[B, (2 d + 1) cells of level lvl]: the coefficient arrays of every member on that level (a view)."""
        if self._strength is None:  # (`fine` and `rebuild` come through here too)
            raise ValueError("EnsembleGMG: only an object made by from_coeffs has `fine`, `level` and `rebuild`")
        return self.coeffs[:, self._offsets[lvl]:self._offsets[lvl + 1]]

    @property
    def fine(self):
        """[B, 2 d + 1, *shape]: the finest coefficient arrays inside the packed hierarchy (a view; `rebuild()` after
        writing them)."""
        return self.level(0).unflatten(1, (2 * self.ndim + 1,) + self.shapes[0])

    def rebuild(self, coeffs=None):
        """The set-up again for new finest coefficients [B, 2 d + 1, *shape] (None: already written into `fine`), into the
        buffers and the launch plan of this object: no device allocation, the same launches as `from_coeffs`.  When the
        members -- all of them -- decide on other axes than before, the hierarchy is planned anew (new buffers); members
        that disagree raise ValueError as in `from_coeffs`, and the coarse levels then hold no valid operator until the next
        successful rebuild."""
        if coeffs is not None:
            assert tuple(coeffs.shape) == tuple(self.fine.shape) and coeffs.dtype == self.dtype
            self.fine.copy_(coeffs)
        nlev = len(self.shapes)
        for lvl in range(nlev):
            halve = self._decide(self.level(lvl), lvl, self.shapes[lvl]) if self._may_coarsen(self.shapes[:lvl + 1]) else None
            if halve != (self.halve[lvl] if lvl + 1 < nlev else None):
                self._plan(self.level(0).clone())  # (other levels than before)
                return self
            if halve is not None:
                ops.stencil_var_coarsen_batch(self.level(lvl), self.shapes[lvl], halve, out=self.level(lvl + 1))
        self._invert(self.level(nlev - 1), self.shapes[-1], self._dense, self.inv)
        return self

    def _run(self, x, b, tol, maxcycles, start, mode):
        assert tuple(x.shape) == tuple(b.shape) == (self.nbatch,) + self.shapes[0], (x.shape, b.shape)
        out = self._out.get(maxcycles)
        if out is None:
            out = self._out[maxcycles] = (
                torch.zeros((self.nbatch, maxcycles + 2), dtype=torch.float64, device=self.device),
                torch.zeros((self.nbatch, 3 if self.krylov == "auto" else 2), dtype=torch.int32, device=self.device))
        self._launch(x, b, out[0], out[1], start, mode, maxcycles, tol)
        # ONE read-back per solve of the whole ensemble, after the launch
        self.history, self.outcome = out[0].cpu().numpy(), out[1].cpu().numpy()
        return x

    def solve(self, b, x, tol=1e-10, maxcycles=60, start=2):
        """A_b x_b = b_b for every member, in place in x [B, *shape] (start 0: from zero, 1: from the content of x, 2: by
        nested iteration) to mean((A x - b)^2) <= tol^2 mean(b^2), at most `maxcycles` cycles each; `status` tells."""
        return self._run(x, b, tol, maxcycles, start, 0)

    def newton_step(self, u, rhs, tol=1e-10, maxcycles=60, start=2):
        """u_b <- u_b - d_b with A_b d_b = A_b u_b - rhs_b for every member, in place in u [B, *shape]."""
        return self._run(u, rhs, tol, maxcycles, start, 1)

    def status(self, member):
        """What `PoissonGMG.solve` reports, for one member of the last launch; handover: the cycle before which the member
        went on with GCR (None: it never did).  Stop reason 4, a breakdown of GCR: converged=False, stagnated=False."""
        k, why = (int(v) for v in self.outcome[member][:2])
        handover = int(self.outcome[member][2]) if self.outcome.shape[1] > 2 and self.outcome[member][2] >= 0 else None
        hist = self.history[member]
        res = math.sqrt(max(float(hist[1 + k]), 0.0) * self.cells) if hist[1 + k] == hist[1 + k] else float("nan")
        bn = math.sqrt(max(float(hist[0]), 0.0) * self.cells) if hist[0] == hist[0] else float("nan")
        return dict(residual=res, bnorm=bn, niter=k, converged=why == 0, stagnated=bool(why == 2 and res < bn),
                    method=self.method if handover is None else "{} + GCR({})".format(self.method, self.krylov_m),
                    handover=handover)


def mean_children(r, loc, out=None):
    """The mean of the merged children: r [..., *shape] -> [..., *shape halved on the 'c' axes of loc] (the R of the
    aggregation-built coarse operators, `StencilGMG.restrict`).  Axis by axis the sum of the even and the odd cells, then
    one scaling: elementwise launches only, so the bits of a member do not depend on what else the array holds."""
    lead = r.dim() - len(loc)
    for a, l in enumerate(loc):
        if l == "c":
            even, odd = [slice(None)] * r.dim(), [slice(None)] * r.dim()
            even[lead + a], odd[lead + a] = slice(0, None, 2), slice(1, None, 2)
            r = r[tuple(even)] + r[tuple(odd)]
    return torch.mul(r, 1.0 / 2 ** loc.count("c"), out=out)


def sweep_plan(weights, first_single=False):
    """The launches of the sweeps with `weights`, in order: tuples of one weight (a single sweep) or two (the one-pass
    pair) -- pairs from the front, a single sweep left over when the count is odd, e.g. [(w0, w1), (w2,)].
    first_single: the first sweep stays a launch of its own (it carries the norm's partial sums), the rest is paired:
    [(w0,), (w1, w2), (w3,)].  Host arithmetic only."""
    weights = list(weights)
    plan = [(weights.pop(0),)] if first_single and weights else []
    while weights:
        plan.append(tuple(weights[:2]))
        weights = weights[2:]
    return plan


class EnsembleLaunchGMG(EnsembleGMG):
    """B systems of ONE shape that are too large for one workgroup each, solved side by side: the hierarchy of
    `EnsembleGMG.from_coeffs` (the same batched set-up, member 0's coarsening decisions, ValueError for a member that
    decides otherwise), split in two.  The finest level and every further level of more than `tail_max_cells` cells are
    LAUNCH levels: each phase of `StencilGMG`'s cycle is one launch there that covers all members (the member on
    blockIdx.y: odil_stencil_var_smooth_batch, odil_stencil_var_residual_restrict_batch, `ops.interp_add` on [B, *shape]).
    The levels below form the TAIL, at most `max_levels` levels down to at most `max_coarsest` unknowns, walked by one
    workgroup per member (odil_stencil_solve_batch).  ValueError naming the levels when they do not split that way.

    The cycle is StencilGMG's: nu1 / nu2 sweeps with `jacobi_weights`, the mean of the merged children down (a transition
    that merges some axes only: the residual, then `mean_children`), `interp_add` up, in 3-D two cycles on level 1.  A
    coarse correction on the tail's top level is odil_stencil_solve_batch with start 0, tol 0 and maxcycles 1 (2 where
    level 1 is the tail's top in 3-D).  A cycle of member b reads its iterate from x and only its LAST post-smoothing
    sweep writes x; everything in between is scratch.  On a launch level that `pair_eligible` admits the sweeps run two per
    pass over the coefficient arrays (odil_stencil_var_smooth2_batch, `sweep_plan`), bit-identical to single sweeps.

    `solve` keeps the contract of `EnsembleGMG.solve` -- start codes, stop rules, `status`, `history`, `outcome` -- with
    the decision on the device: the first pre-smoothing sweep of cycle k leaves partial sums of (A x_k - b)^2, and
    odil_stencil_cycle_decide_batch turns them into history[b, 1 + k], applies the stop rules and clears active[b] of a
    member that stops.  Every later launch skips such a member whole, so its x stays x_k.  The host reads ONE int per cycle,
    the number of active members (copied while the rest of the cycle runs), and nothing else until `history` and `outcome`
    after the solve.  FROZEN MEMBERS STILL RUN THROUGH THE TAIL LAUNCH and through `interp_add` (neither can skip
    members); what these compute for them lands in scratch and is discarded.  A member's iterate, history and outcome do
    not depend on nbatch, on its position, or on when other members stop.

    Attributes as `EnsembleGMG.core`; besides: nlaunch (number of launch levels), tail_shapes.  `newton_step` is not
    served (the Newton driver solves M d = f and updates on its own).  The hand-over to GCR of `EnsembleGMG(krylov="auto")`
    -- inside ONE launch -- is not served in this form: krylov other than "never" raises ValueError.  The subclass
    `EnsembleLaunchKrylovGMG` hands slow members to GCR across the launches (`optimize_newton_ensemble(krylov="any")`)."""

    tail_max_cells = EnsembleGMG.max_cells  # levels of at most this many cells go to the one-workgroup tail (never the finest)
    method_name = "gmg-vcycle (variable coefficients), batched launches"
    max_member_cells = 1 << 24  # (the member is a grid dimension of the batched launches: their limit per member)
    pair_min_cells = 1 << 20  # launch levels on which ALL members together have at least this many cells smooth in pairs (odil_stencil_var_smooth2_batch); math.inf: single sweeps only.  Measured: the largest of 2^18 ... 2^23 that loses on no row of the table

    def __init__(self, coeffs, nu1=None, nu2=None, min_size=2, tail_max_cells=None, krylov="never"):
        if krylov != "never":
            raise ValueError("EnsembleLaunchGMG: krylov '{}' (the batched launches have no hand-over to GCR: 'never' "
                             "only)".format(krylov))
        self._strength = None
        self._set_krylov("never", 6)
        self.method = self.method_name
        if tail_max_cells is not None:
            self.tail_max_cells = int(tail_max_cells)
        for name, nu in (("nu1", nu1), ("nu2", nu2)):
            if nu is not None and not 1 <= nu <= 4:
                raise ValueError("EnsembleLaunchGMG: {} = {} (1..4 sweeps: the first one carries the norm, the tail takes at "
                                 "most 4)".format(name, nu))
        self._init_coeffs(coeffs, nu1, nu2, min_size)

    @classmethod
    def from_coeffs(cls, coeffs, nu1=None, nu2=None, min_size=2, tail_max_cells=None, krylov="never"):
        """coeffs [B, 2 d + 1, *shape]; tail_max_cells: None for the class's; krylov: 'never' (else ValueError)."""
        return cls(coeffs, nu1=nu1, nu2=nu2, min_size=min_size, tail_max_cells=tail_max_cells, krylov=krylov)

    @classmethod
    def split(cls, shapes, tail_max_cells=None):
        """The number of launch levels of a hierarchy `shapes` (fine to coarse): the finest, and the further levels while
        they have more than tail_max_cells cells; the rest is the tail.  ValueError naming the levels when there is no tail,
        or one workgroup does not walk it (host arithmetic only)."""
        limit = cls.tail_max_cells if tail_max_cells is None else tail_max_cells
        shapes = [tuple(int(n) for n in s) for s in shapes]
        first = next((l for l in range(1, len(shapes)) if math.prod(shapes[l]) <= limit), len(shapes))
        tail = shapes[first:]
        if not tail:
            raise ValueError("EnsembleLaunchGMG: levels {} have no level of at most {} cells below the finest for the "
                             "one-workgroup tail".format(shapes, limit))
        if len(tail) > cls.max_levels or math.prod(tail[-1]) > cls.max_coarsest:
            raise ValueError("EnsembleLaunchGMG: the tail {} of the levels {} is not walked by one workgroup (at most {} "
                             "levels, a coarsest level of at most {} unknowns)".format(tail, shapes, cls.max_levels,
                                                                                      cls.max_coarsest))
        return first

    @classmethod
    def plan(cls, shape, tail_max_cells=None, min_size=2):
        """(launch shapes, tail shapes) of members whose every transition merges every axis (what coefficients of equal
        strength along the axes decide): StencilGMG's rule, stopped where the tail has `max_levels` levels.  Host
        arithmetic only; ValueError as `split`."""
        limit = cls.tail_max_cells if tail_max_cells is None else tail_max_cells
        shapes = [tuple(int(n) for n in shape)]
        while cls._tail_room(shapes, limit) and all(n % 2 == 0 and n // 2 >= min_size for n in shapes[-1]):
            shapes.append(tuple(n // 2 for n in shapes[-1]))
        first = cls.split(shapes, limit)
        return shapes[:first], shapes[first:]

    @classmethod
    def _tail_room(cls, shapes, limit):
        first = next((l for l in range(1, len(shapes)) if math.prod(shapes[l]) <= limit), len(shapes))
        return len(shapes) - first < cls.max_levels

    def _check_fine(self, shape):
        if math.prod(shape) > self.max_member_cells:
            raise ValueError("EnsembleLaunchGMG.from_coeffs: {} cells per member are above the limit of the batched launches "
                             "({})".format(math.prod(shape), self.max_member_cells))

    def _may_coarsen(self, shapes):
        return self._tail_room(shapes, self.tail_max_cells)

    def _pack(self, levels):
        """(rows of an even number of elements: the batched residual + restriction reads cell pairs as aligned packs)"""
        row = sum(level.shape[1] for level in levels)
        if row % 2:
            levels = levels + [torch.zeros((self.nbatch, 1), dtype=self.dtype, device=self.device)]
        return torch.cat(levels, dim=1).contiguous()

    def _work_elements(self, shapes):
        first = self.split(shapes, self.tail_max_cells)
        need = ops.stencil_solve_batch_work(shapes[first:])
        if not need:
            raise ValueError("EnsembleLaunchGMG: the tail {} is not walked by one workgroup".format(shapes[first:]))
        return need

    def _finish(self, shapes, halves, coeffs, inv):
        need = self._work_elements(shapes)
        nb, dtype, device = self.nbatch, self.dtype, self.device
        self.shapes, self.halve = shapes, halves
        self.locs = ["".join("c" if on else "." for on in halve) for halve in halves]
        self.coeffs, self.inv, self.cells = coeffs, inv, math.prod(shapes[0])
        self.nlaunch = first = self.split(shapes, self.tail_max_cells)
        self.tail_shapes = shapes[first:]
        self.work = torch.empty((nb, need), dtype=dtype, device=device)
        self._plan_tail()

        def arrays(lvl):
            return torch.zeros((nb,) + shapes[lvl], dtype=dtype, device=device)

        # per launch level: iterate (level 0: the caller's x), right-hand side (level 0: the caller's b), two scratch
        # arrays; the tail's top level: iterate and right-hand side
        self._x = [None] + [arrays(l) for l in range(1, first + 1)]
        self._b = [None] + [arrays(l) for l in range(1, first + 1)]
        self._s = [(arrays(l), arrays(l)) for l in range(first)]
        nparts = ops.stencil_var_smooth_batch_parts(shapes[0])
        self._partials = torch.zeros((nb, nparts), dtype=torch.float64, device=device)
        self._partials0 = torch.zeros((nb, nparts), dtype=torch.float64, device=device)
        self._active = torch.ones(nb, dtype=torch.int32, device=device)
        self._nactive = torch.zeros(1, dtype=torch.int32, device=device)
        self._nactive_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._decided = torch.cuda.Event()
        self._tail_out = (torch.zeros((nb, 4), dtype=torch.float64, device=device),
                          torch.zeros((nb, 2), dtype=torch.int32, device=device))
        self._out = dict()
        self.history = None
        self.outcome = None
        missing = [name for name in self.core if not hasattr(self, name)]
        assert not missing, "EnsembleLaunchGMG lacks {}".format(missing)

    def _plan_tail(self):
        """The launch plan of the tail (odil_stencil_solve_batch) from the object's levels, weights and coarsest inverses."""
        first = self.nlaunch
        sizes = [(2 * self.ndim + 1) * math.prod(s) for s in self.shapes]
        tail_coeffs = self.coeffs[:, sum(sizes[:first]):sum(sizes)]
        self._launch = ops.stencil_solve_batch_plan(tail_coeffs, self.tail_shapes, self.halve[first:], self.nbatch, self.work,
                                                    self.inv, self.wpre, self.wpost)

    def _tail_solve(self, start, maxcycles):
        """The tail's top level: x <- its nested-iteration start (start 2, maxcycles 0) or `maxcycles` cycles from zero
        (start 0), for every member, frozen ones included (their result is discarded)."""
        top = self.nlaunch
        self._launch(self._x[top], self._b[top], self._tail_out[0], self._tail_out[1], start, 0, maxcycles, 0.0)
        return self._x[top]

    def pair_eligible(self, lvl):
        """Launch level lvl smooths in pairs (odil_stencil_var_smooth2_batch): a shape the pair admits, and at least
        `pair_min_cells` cells of ALL members together on that level (together they fill the chip).  Host arithmetic."""
        return (ops.smooth2_supported(self.shapes[lvl])
                and self.nbatch * math.prod(self.shapes[lvl]) >= self.pair_min_cells)

    def _launches(self, lvl, weights, first_single=False):
        """`sweep_plan` on a level that pairs, else one launch per sweep (the cycle without the pair kernel)."""
        return sweep_plan(weights, first_single) if self.pair_eligible(lvl) else [(w,) for w in weights]

    def _smooth(self, c, src, b, ws, dst, partials=None, mask=None):
        """One launch of the plan: a single sweep (with the partial sums, where asked for) or the one-pass pair."""
        mask = self._active if mask is None else mask
        if len(ws) == 2:
            ops.stencil_var_smooth2_batch(c, src, b, ws[0], ws[1], dst, active=mask)
        else:
            ops.stencil_var_smooth_batch(c, src, b, ws[0], dst, active=mask, partials=partials)

    def _cycle(self, lvl, x, b, zero=False, decide=None, mask=None):
        """One cycle of every active member on launch level lvl, from x (zero: from the zero vector) into x.
        decide: called after the first pre-smoothing sweep, which then leaves its partial sums; True ends the cycle there.
        mask: int32 [B], the members the launches serve (None: the active ones).
        Sweeps run in the launches of `sweep_plan` where the level pairs (bit-identical to single sweeps); every launch
        but the last one of the post-smoothing writes one of the two scratch arrays, never the one it reads."""
        c, active = self.level(lvl), self._active if mask is None else mask
        scratch = self._s[lvl]
        cur = None if zero else x
        pre = self._launches(lvl, self.wpre, first_single=decide is not None)
        for j, ws in enumerate(pre):
            dst = scratch[j % 2]
            self._smooth(c, cur, b, ws, dst, partials=self._partials if decide is not None and j == 0 else None, mask=active)
            cur = dst
            if decide is not None and j == 0 and decide():
                return
        other = scratch[len(pre) % 2]
        bc = self._b[lvl + 1]
        if all(self.halve[lvl]):
            ops.stencil_var_residual_restrict_batch(c, cur, b, 1.0 / 2 ** self.ndim, bc, active=active)
        else:
            ops.stencil_var_smooth_batch(c, cur, b, 0.0, other, mode=1, active=active)
            mean_children(other, self.locs[lvl], out=bc)
        twice = lvl == 0 and self.ndim == 3 and len(self.shapes) > 2  # (`StencilGMG.finish_cycle`)
        if lvl + 1 == self.nlaunch:
            xc = self._tail_solve(0, 2 if twice else 1)
        else:
            xc = self._x[lvl + 1]
            self._cycle(lvl + 1, xc, bc, zero=True, mask=active)
            if twice:
                self._cycle(lvl + 1, xc, bc, mask=active)
        ops.interp_add(xc, "." + self.locs[lvl], add=cur, out=other)  # x + P x_c
        cur, other = other, cur
        post = self._launches(lvl, self.wpost)
        for j, ws in enumerate(post):
            dst = x if j == len(post) - 1 else other
            self._smooth(c, cur, b, ws, dst, mask=active)
            cur, other = dst, cur

    def _nested(self, b, x):
        """The nested-iteration start into x: b restricted down the launch levels, the tail's own start on its top level,
        then every launch level one cycle from the interpolated solution of the level below."""
        for lvl in range(self.nlaunch):
            mean_children(b if lvl == 0 else self._b[lvl], self.locs[lvl], out=self._b[lvl + 1])
        self._tail_solve(2, 0)
        for lvl in range(self.nlaunch - 1, -1, -1):
            xl, bl = (x, b) if lvl == 0 else (self._x[lvl], self._b[lvl])
            ops.interp_add(self._x[lvl + 1], "." + self.locs[lvl], out=xl)
            self._cycle(lvl, xl, bl)

    def solve(self, b, x, tol=1e-10, maxcycles=60, start=2):
        """`EnsembleGMG.solve`: A_b x_b = b_b for every member, in place in x [B, *shape] (contiguous, as b)."""
        assert tuple(x.shape) == tuple(b.shape) == (self.nbatch,) + self.shapes[0], (x.shape, b.shape)
        assert x.is_contiguous() and b.is_contiguous() and x.dtype == b.dtype == self.dtype and start in (0, 1, 2)
        out = self._out.get(maxcycles)
        if out is None:
            out = self._out[maxcycles] = (
                torch.zeros((self.nbatch, maxcycles + 2), dtype=torch.float64, device=self.device),
                torch.zeros((self.nbatch, 2), dtype=torch.int32, device=self.device))
        history, outcome = out
        self._active.fill_(1)
        if start == 0:
            x.zero_()  # (what a member keeps that stops before its first cycle)
            bsq = self._partials  # (the first sweep starts from zero: its partial sums are those of b^2)
        else:
            if start == 2:
                self._nested(b, x)
            # (b^2 by a sweep from zero into scratch: three words per cell, once per solve)
            bsq = self._partials0
            ops.stencil_var_smooth_batch(self.level(0), None, b, 1.0, self._s[0][0], partials=bsq)
        for k in range(maxcycles + 1):
            def decide():
                ops.stencil_cycle_decide_batch(self._partials, self.cells, k, maxcycles, tol, history, outcome, self._active,
                                               self._nactive, partials0=bsq if k == 0 else None)
                self._nactive_host.copy_(self._nactive, non_blocking=True)
                self._decided.record()
                return k == maxcycles  # (every member stops there at the latest: nothing of this cycle is left to run)

            self._cycle(0, x, b, zero=start == 0 and k == 0, decide=decide)
            self._decided.synchronize()  # (ONE int per cycle; the rest of the cycle is in flight meanwhile)
            if int(self._nactive_host[0]) == 0:
                break
        # ONE read-back of history and outcome per solve of the whole ensemble
        self.history, self.outcome = history.cpu().numpy(), outcome.cpu().numpy()
        return x

    def newton_step(self, u, rhs, tol=1e-10, maxcycles=60, start=2):
        raise ValueError("EnsembleLaunchGMG: newton_step is not served (solve M d = f with `solve`, then update)")


class EnsembleLaunchKrylovGMG(EnsembleLaunchGMG):
    """`EnsembleLaunchGMG` with the hand-over of `EnsembleGMG(krylov="auto")`: a member whose cycles stop contracting goes
    on with GCR(krylov_m) around the same batched cycle, ACROSS the launches, every decision on the device
    (odil_stencil_gcr_*_batch; decision order, pass algebra and stop reasons: odil_stencil_solve_krylov_batch).

    One lock-step loop of passes; pass k is the same pass for all members.  A member is STATIONARY (the base class's cycle,
    launch for launch, under the mask `active`), in GCR (after its hand-over) or stopped.  Per pass:
      the first pre-smoothing sweep of the stationary members, then the decision (mode 0): a stationary member under the
        base class's rules plus the HAND-OVER -- it keeps x_k, since only the masked last post-smoothing sweep writes x --
        and a GCR member on the mean(rho^2) its last pass left as history[1 + k];
      the rest of the stationary cycle;
      the host reads FOUR ints (stationary, GCR, to verify, rho to form; copied while the cycle runs) and enqueues only
        the sequences that have members: rho = b - A x for the members handed over or to verify; the true residual's norm
        and the decision of the members to verify (mode 3: converged only on the TRUE residual, else GCR restarts from it);
        the GCR sequence: e = one cycle from the zero start on rho under the mask `gcr` (the base class's launches on the
        same scratch), t = 0 - A e, the products with the kept Q_j, the betas (mode 1), the projection of (q, z), the
        scaling 1 / |q| and a = <q, rho> or the BREAKDOWN (mode 2), then x += a z, rho -= a q.
    Pass k works in the rows k mod krylov_m of the store [B, 2 krylov_m, cells]: the cycle writes e and the residual
    launch t straight into them, the projection and the scaling run in place.  After krylov_m passes the directions are
    dropped.  The tail launch and `interp_add` cannot skip members: what they compute for masked-out members lands in
    scratch and is discarded.  The loop runs at most maxcycles + 1 passes.  An ensemble in which no member hands over makes
    the launches of `EnsembleLaunchGMG` (with the wider decision kernel) and nothing more: x, history and (passes, reason)
    are its bits.  A member's bits do not depend on nbatch, its position, or what other members do.

    krylov == "auto" as an attribute: `status` and the [B, 3] `outcome` (passes, reason, hand-over cycle or -1) of
    `EnsembleGMG` apply unchanged.  Work memory: (2 krylov_m + 2) finest-level vectors per member (store, rho, and a zero
    vector).  (`_set_cycle` is a hook of the tests.)"""

    def __init__(self, coeffs, nu1=None, nu2=None, min_size=2, tail_max_cells=None, krylov_m=6):
        if not 1 <= int(krylov_m) <= 8:
            raise ValueError("EnsembleLaunchKrylovGMG: krylov_m = {} (1..8 directions)".format(krylov_m))
        self._m = int(krylov_m)
        super().__init__(coeffs, nu1=nu1, nu2=nu2, min_size=min_size, tail_max_cells=tail_max_cells)
        self.krylov, self.krylov_m = "auto", self._m

    @classmethod
    def from_coeffs(cls, coeffs, nu1=None, nu2=None, min_size=2, tail_max_cells=None, krylov_m=6):
        """coeffs [B, 2 d + 1, *shape]; tail_max_cells: None for the class's; krylov_m: 1..8 directions (else ValueError)."""
        return cls(coeffs, nu1=nu1, nu2=nu2, min_size=min_size, tail_max_cells=tail_max_cells, krylov_m=krylov_m)

    def _finish(self, shapes, halves, coeffs, inv):
        super()._finish(shapes, halves, coeffs, inv)
        self._gcr = ops.GcrBatch(self.nbatch, shapes[0], self._m, self.dtype, self.device, self._active)

    def _set_cycle(self, wpre=None, wpost=None, inv=None):
        """A TEST HOOK, not part of the supported surface: other sweep weights (as many as before) and / or coarsest
        inverses [B, n, n] for every later cycle -- how a test makes the cycle return nothing (weights 0, inverse 0) to
        reach the breakdown of GCR with a numerical input.  ValueError for another number of weights or another shape."""
        for name, new, old in (("wpre", wpre, self.wpre), ("wpost", wpost, self.wpost)):
            if new is not None and len(new) != len(old):
                raise ValueError("EnsembleLaunchKrylovGMG._set_cycle: {} weights for {} ({} sweeps)".format(
                    len(new), name, len(old)))
        if inv is not None and tuple(inv.shape) != tuple(self.inv.shape):
            raise ValueError("EnsembleLaunchKrylovGMG._set_cycle: inverses {} (the object's: {})".format(
                tuple(inv.shape), tuple(self.inv.shape)))
        if wpre is not None:
            self.wpre = [float(w) for w in wpre]
        if wpost is not None:
            self.wpost = [float(w) for w in wpost]
        if inv is not None:
            self.inv.copy_(inv)
        self._plan_tail()
        return self

    def solve(self, b, x, tol=1e-10, maxcycles=60, start=2):
        """`EnsembleGMG.solve`: A_b x_b = b_b for every member, in place in x [B, *shape] (contiguous, as b)."""
        assert tuple(x.shape) == tuple(b.shape) == (self.nbatch,) + self.shapes[0], (x.shape, b.shape)
        assert x.is_contiguous() and b.is_contiguous() and x.dtype == b.dtype == self.dtype and start in (0, 1, 2)
        out = self._out.get(maxcycles)
        if out is None:
            out = self._out[maxcycles] = (
                torch.zeros((self.nbatch, maxcycles + 2), dtype=torch.float64, device=self.device),
                torch.zeros((self.nbatch, 3), dtype=torch.int32, device=self.device))
        history, outcome = out
        g, m, fine = self._gcr, self._m, self.level(0)
        self._active.fill_(1)
        g.reset()
        outcome[:, 2].fill_(-1)
        if start == 0:
            x.zero_()
            bsq = self._partials
        else:
            if start == 2:
                self._nested(b, x)
            bsq = self._partials0
            ops.stencil_var_smooth_batch(fine, None, b, 1.0, self._s[0][0], partials=bsq)
        nstat = self.nbatch
        for k in range(maxcycles + 1):
            def decide():
                g.decide(0, k, maxcycles, tol, history, outcome, self._partials, partials0=bsq if k == 0 else None)
                g.counts_host.copy_(g.counts, non_blocking=True)
                self._decided.record()
                return k == maxcycles

            if nstat:
                self._cycle(0, x, b, zero=start == 0 and k == 0, decide=decide)
            else:
                decide()
            self._decided.synchronize()  # (FOUR ints per pass; the stationary cycle is in flight meanwhile)
            nstat, ngcr, nverify, nfresh = (int(v) for v in g.counts_host)
            if nstat + ngcr + nverify == 0:
                break
            if nfresh:  # (handed over before this pass, or to verify)
                ops.stencil_var_smooth_batch(fine, x, b, 0.0, g.rho, mode=1, active=g.fresh)
            if nverify:
                g.sumsq(g.rho, g.verify)
                g.decide(3, k, maxcycles, tol, history, outcome, self._partials)
            if (ngcr or nverify) and k < maxcycles:
                slot = k % m
                e, t = g.row(slot), g.row(m + slot)
                self._cycle(0, e, g.rho, zero=True, mask=g.gcr)
                ops.stencil_var_smooth_batch(fine, e, g.zero, 0.0, t, mode=1, active=g.gcr)
                g.dots(slot)
                g.decide(1, k, maxcycles, tol, history, outcome, self._partials)
                g.project(slot)
                g.decide(2, k, maxcycles, tol, history, outcome, self._partials)
                g.update(slot, x)
        # ONE read-back of history and outcome per solve of the whole ensemble
        self.history, self.outcome = history.cpu().numpy(), outcome.cpu().numpy()
        return x

    def newton_step(self, u, rhs, tol=1e-10, maxcycles=60, start=2):
        raise ValueError("EnsembleLaunchKrylovGMG: newton_step is not served (solve M d = f with `solve`, then update)")


def stencil_coefficients(items, shape, period=None, dtype=None, device=None):
    """The coefficient tensor [(2 d + 1), *shape] (order 0, -e_0, +e_0, -e_1, ...) of a Jacobian given as `items` =
    [(shift, coefficient array of `shape`)], or None when a shift is neither 0 nor a unit vector or the centre is missing.
    Shifts are taken modulo `period` (the extents of the periodic roll; default `shape`: |shift| <= n / 2).  Shifts that do
    not occur are zero arrays, duplicates are summed.  Arrays that already lie back to back in the wanted order (the
    generated Jacobian kernel writes slices of one buffer in the order the operator reads them) give a view, no copies."""
    ndim = len(shape)
    period = tuple(period) if period is not None else tuple(shape)
    want = [(0,) * ndim]
    for i in range(ndim):
        want += [tuple(-1 if j == i else 0 for j in range(ndim)), tuple(1 if j == i else 0 for j in range(ndim))]
    norms = [tuple(((s + n // 2) % n) - n // 2 for s, n in zip(shift, period)) for shift, _ in items]
    if any(norm not in want for norm in norms) or want[0] not in norms:
        return None
    if len(set(norms)) == len(norms) == len(want):
        arrs = [items[norms.index(sft)][1] for sft in want]
        first, size = arrs[0], arrs[0].numel()
        if all(a.is_contiguous() and a.dtype == first.dtype and a.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
               and a.storage_offset() == first.storage_offset() + j * size for j, a in enumerate(arrs)):
            return torch.empty(0, dtype=first.dtype, device=first.device).set_(
                first.untyped_storage(), first.storage_offset(), (len(want),) + tuple(shape))
    coeffs = torch.zeros((len(want),) + tuple(shape), dtype=dtype or items[0][1].dtype, device=device or items[0][1].device)
    seen = set()
    for norm, (_, coeff) in zip(norms, items):
        slot = want.index(norm)
        if slot in seen:
            ops.axpy(coeffs[slot].view(-1), coeff.reshape(-1).contiguous(), 1.0)
        else:
            coeffs[slot].view(-1).copy_(coeff.reshape(-1))
            seen.add(slot)
    return coeffs


SlotPlan = collections.namedtuple("SlotPlan", "slots missing single")


def stencil_slot_plan(jac_items, shape, fields=None):
    """Where the arrays of a generated Jacobian kernel (`_Codegen.jac_items`: (output, None) for the value of an output,
    (output, (key, shift, loc, frozen)) for d output / d read) go in the layout of `stencil_coefficients`, decided on the
    host once: SlotPlan(slots, missing, single).  slots[j]: None for the value (it goes to the residual array), else the
    slot 0, -e_0, +e_0, -e_1, ... of [2 d + 1, *shape]; missing: the slots no item writes (zero arrays); single: None when
    the items land in distinct slots -- the kernel may then write straight into the packed arrays -- else the reason why
    the arrays must pass through `stencil_coefficients` (duplicate normalised shifts are summed there).
    The checks are those of `recognise_stencil`, and what it answers with None raises ValueError here: one output, one
    plain cell-centred field (fields: {key: location} of the state's fields, when known), d <= 3, extents >= 4, every shift
    0 or a unit vector modulo the extents, the centre present."""
    shape = tuple(int(n) for n in shape)
    ndim = len(shape)
    if fields is not None and (len(fields) != 1 or next(iter(fields.values())) != "c" * ndim):
        raise ValueError("not one cell-centred field: {}".format(dict(fields)))
    if ndim > 3 or any(n < 4 for n in shape):
        raise ValueError("grid {}: at most three dimensions, extents of at least 4".format(shape))
    if {k for k, _ in jac_items} != {0} or sum(attr is None for _, attr in jac_items) != 1:
        raise ValueError("{} outputs (one residual array is needed)".format(len({k for k, _ in jac_items})))
    want = [(0,) * ndim]
    for i in range(ndim):
        want += [tuple(-1 if j == i else 0 for j in range(ndim)), tuple(1 if j == i else 0 for j in range(ndim))]
    slots, keys = [], set()
    for _, attr in jac_items:
        if attr is None:
            slots.append(None)
            continue
        key, shift, loc = attr[:3]
        keys.add(key)
        norm = tuple(((int(s) + n // 2) % n) - n // 2 for s, n in zip(shift, shape))
        if loc != "c" * ndim or len(shift) != ndim or norm not in want:
            raise ValueError("the read of '{}' at shift {} ({}) is not a point of the (2 d + 1)-point stencil".format(
                key, tuple(shift), loc))
        slots.append(want.index(norm))
    if len(keys) != 1 or 0 not in slots:
        raise ValueError("no derivative with respect to the cell itself" if len(keys) == 1 else
                         "derivatives with respect to {} fields".format(len(keys)))
    used = [s for s in slots if s is not None]
    single = None
    if len(set(used)) != len(used):
        twice = next(s for s in used if used.count(s) > 1)
        single = "{} reads at the normalised shift {}: their coefficient arrays are summed".format(used.count(twice), want[twice])
    return SlotPlan(slots, [s for s in range(len(want)) if s not in used], single)


def recognise_stencil(op):
    """The coefficient tensor [(2 d + 1), *shape] (order 0, -e_0, +e_0, -e_1, ...) when the LinearizedOperator is square,
    acts on ONE cell-centred `Field` (d <= 3, extents >= 4) and every stencil block's shift is 0 or a unit vector --
    the structure StencilGMG needs; None otherwise (`stencil_coefficients`)."""
    from .core import Field

    if len(op.key_to_field) != 1 or op.nrows != op.ncols:
        return None
    (key, field), = op.key_to_field.items()
    if not isinstance(field, Field):
        return None
    shape = tuple(field.array.shape)
    ndim = len(shape)
    if ndim > 3 or field.loc != "c" * ndim or any(s < 4 for s in shape):
        return None
    items = []
    for row0, nrows, kind, k, payload in op.blocks:
        if kind != "stencil" or row0 != 0 or nrows != op.ncols:
            return None
        coeff, shift, loc, vshape = payload
        if loc != field.loc or tuple(vshape) != shape:
            return None
        items.append((shift, coeff))
    if not items:
        return None
    return stencil_coefficients(items, shape, dtype=op.dtype, device=op.device)


def recognise_poisson(op):
    """(shape, h2) if the LinearizedOperator is exactly the zero-Dirichlet Laplacian stencil of one
    cell-centred field, else None."""
    from .core import Field

    if len(op.key_to_field) != 1 or op.nrows != op.ncols:
        return None
    (key, field), = op.key_to_field.items()
    if not isinstance(field, Field):
        return None
    shape = tuple(field.array.shape)
    ndim = len(shape)
    if ndim > 3 or field.loc != "c" * ndim or any(s < 2 for s in shape):
        return None
    blocks = {}
    for row0, nrows, kind, k, payload in op.blocks:
        if kind != "stencil" or row0 != 0 or nrows != op.ncols:
            return None
        coeff, shift, loc, vshape = payload
        if loc != field.loc or tuple(vshape) != shape or shift in blocks:
            return None
        blocks[shift] = coeff
    want = [(0,) * ndim]
    for i in range(ndim):
        want += [tuple(-1 if j == i else 0 for j in range(ndim)), tuple(1 if j == i else 0 for j in range(ndim))]
    if sorted(blocks) != sorted(want):
        return None
    npdt = np.float64 if op.dtype == torch.float64 else np.float32
    h2 = [npdt(op.domain.step_by_dim(i)) ** 2 for i in range(ndim)]
    rtol = 1e-11 if op.dtype == torch.float64 else 1e-4
    # ONE pass over the coefficient arrays against the values the Poisson Jacobian has there (formed on the fly: no
    # reference arrays), one read-back
    pairs = ops.poisson_jac_match([blocks[shift] for shift in want], shape, h2).cpu().numpy()
    if not np.all(pairs[:, 0] <= rtol * pairs[:, 1]):  # (NaN compares false)
        return None
    return shape, h2


# ======================================================================================================================
# Multigrid for the damped normal equations of several grid fields (csrc/block_mg.hip)
# ======================================================================================================================
# Host planning (numpy, no device): the index maps of `Context.field`, the offset pattern of A = M^T M and of the
# coarse operators.  Shapes are canonical 3-D (leading axes of extent 1).

COARSEST_MAX_UNKNOWNS = 4096  # the coarsest level is solved exactly (a dense pseudo-inverse)
MAX_FIELDS = 8  # fields per level descriptor: kBmgMaxFields in csrc/block_mg.hip


def canon3(shape):
    return (1,) * (3 - len(shape)) + tuple(int(s) for s in shape)


def gather_map(sn, field_loc, loc, shift):
    """Row r of the output grid reads field index g[r] along one axis, -1 where it reads the padded constant 0: the map
    of odil_field_gather (pad 'c' -> 'n', periodic roll by -shift, trim 'n' -> 'c'; reference core.py:955-969)."""
    pad = 1 if (field_loc == "c" and loc == "n") else 0
    trim = 1 if (field_loc == "n" and loc == "c") else 0
    nper = sn + pad
    r = np.arange(nper - trim, dtype=np.int64)
    return (r + int(shift) % nper) % nper - pad


def pair_axis_tables(sa, g1, g2):
    """One axis of the term c1 c2 of two blocks that read fields a (extent sa, map g1) and b (map g2) from the same rows:
    {offset o: rmap} with rmap[j] the row that reads a at j and b at j + o, else -1."""
    rows = np.full(sa, -1, dtype=np.int64)
    ok = g1 >= 0
    rows[g1[ok]] = np.nonzero(ok)[0]
    k = np.where(rows >= 0, g2[np.maximum(rows, 0)], -1)
    valid = (rows >= 0) & (k >= 0)
    off = k - np.arange(sa)
    return {int(o): np.where(valid & (off == o), rows, -1) for o in np.unique(off[valid])}


def p1d(code, nf, nc):
    """The 1-D prolongation (nf x nc) of transfer code 0 (identity), 1 (cells: 3/4, 1/4, all of the parent at a wall) or
    2 (nodes: coarse node I on fine node 2 I, linear) -- the weights of pw1 in csrc/block_mg.hip."""
    p = np.zeros((nf, nc))
    for i in range(nf):
        if code == 0:
            p[i, i] = 1.0
        elif code == 2:
            if i % 2 == 0:
                p[i, i // 2] = 1.0
            else:
                p[i, i // 2] = p[i, i // 2 + 1] = 0.5
        else:
            par = i // 2
            nb = par + 1 if i % 2 else par - 1
            if 0 <= nb < nc:
                p[i, par], p[i, nb] = 0.75, 0.25
            else:
                p[i, par] = 1.0
    return p


_p1d_cache = dict()


def _p1d(code, nf, nc):
    key = (code, nf, nc)
    if key not in _p1d_cache:
        _p1d_cache[key] = p1d(code, nf, nc)
    return _p1d_cache[key]


def coarse_axis_offsets(code_a, nfa, nca, code_b, nfb, ncb, o):
    """The offsets J - I at which the 1-D product P_a^T S_o P_b (S_o: k = i + o) is nonzero."""
    pa, pb = _p1d(code_a, nfa, nca), _p1d(code_b, nfb, ncb)
    i = np.arange(nfa)
    ok = (i + o >= 0) & (i + o < nfb)
    if not ok.any():
        return []
    prod = (pa[ok] != 0).astype(np.float64).T @ (pb[i[ok] + o] != 0).astype(np.float64)
    ii, jj = np.nonzero(prod)
    return sorted(set(int(v) for v in (jj - ii)))


def coarse_shape3(shape, codes):
    return tuple(n if c == 0 else n // 2 if c == 1 else (n - 1) // 2 + 1 for n, c in zip(shape, codes))


def plan_levels(cshape, locs, max_coarsest=COARSEST_MAX_UNKNOWNS):
    """Per level the canonical field shapes and, per transition, the transfer codes (3 per field).  An axis is halved
    while its cell count is even; the hierarchy stops at the first level with at most `max_coarsest` unknowns.  None when
    it cannot get there, or when there would be only one level."""
    cells = list(canon3(cshape))
    loc3 = ["." * (3 - len(l)) + l for l in locs]
    shapes = [[tuple(1 if ch == "." else (cells[d] + (1 if ch == "n" else 0)) for d, ch in enumerate(l)) for l in loc3]]
    codes = []
    while sum(math.prod(s) for s in shapes[-1]) > max_coarsest or len(shapes) == 1:
        halve = [d >= 3 - len(cshape) and cells[d] % 2 == 0 and cells[d] >= 2 for d in range(3)]
        if not any(halve):
            return None
        cells = [c // 2 if h else c for c, h in zip(cells, halve)]
        code = [[0 if (not halve[d] or l[d] == ".") else (1 if l[d] == "c" else 2) for d in range(3)] for l in loc3]
        shapes.append([coarse_shape3(s, c) for s, c in zip(shapes[-1], code)])
        codes.append(code)
    return shapes, codes


def level_desc(shapes, ebeg):
    """The host descriptor of a level (include/odil_hip.h: odil_bmg_apply)."""
    offs = [0]
    for s in shapes:
        offs.append(offs[-1] + math.prod(s))
    vals = [len(shapes)] + offs + [v for s in shapes for v in s] + list(ebeg)
    return ops.i64(vals), offs


def normal_pattern(op):
    """The terms of A = M^T M of a LinearizedOperator whose unknowns are all grid fields: a list of
    (a, b, o, block 1, block 2, rmap) in the order of op.blocks (rmap: per axis, concatenated), and the field keys.
    None when a block is dense or a field has a shape this form does not cover."""
    from .core import Field

    keys = list(op.key_to_field)
    ndim = op.domain.ndim
    if ndim > 3:
        return None
    fshape = dict()
    for key, field in op.key_to_field.items():
        if not isinstance(field, Field) or field.loc is None or len(field.loc) != ndim or any(ch not in "cn" for ch in field.loc):
            return None
        shape = tuple(field.array.shape)
        want = tuple(c + (1 if ch == "n" else 0) for c, ch in zip(op.domain.cshape, field.loc))
        if shape != want or op.key_to_size[key] != math.prod(shape):
            return None
        fshape[key] = canon3(shape)
    groups = dict()
    for blk in op.blocks:
        row0, nrows, kind, key, payload = blk
        if kind != "stencil" or key not in fshape:
            return None
        groups.setdefault(row0, []).append(blk)
    terms = []
    for row0, blks in groups.items():
        maps = []
        for _, _, _, key, (coeff, shift, loc, vshape) in blks:
            field = op.key_to_field[key]
            if len(vshape) != ndim:
                return None
            lead = [np.zeros(1, dtype=np.int64)] * (3 - ndim)
            maps.append(lead + [gather_map(int(n), fl, l, s) for n, fl, l, s in zip(field.array.shape, field.loc, loc, shift)])
        for i1, b1 in enumerate(blks):
            a = keys.index(b1[3])
            for i2, b2 in enumerate(blks):
                b = keys.index(b2[3])
                axes = [pair_axis_tables(fshape[b1[3]][d], maps[i1][d], maps[i2][d]) for d in range(3)]
                for o0, r0 in axes[0].items():
                    for o1, r1 in axes[1].items():
                        for o2, r2 in axes[2].items():
                            rmap = np.concatenate([r0, r1, r2])
                            terms.append((a, b, (o0, o1, o2), b1, b2, rmap, canon3(b1[4][3])))
    return terms, keys, [fshape[k] for k in keys]


def coarse_pattern(entries, shapes_f, shapes_c, code):
    """Offsets of the coarse entries P_a^T C_ab P_b from the fine entries [(a, b, o)], sorted (a, b, o)."""
    out = set()
    for a, b, o in entries:
        per = [coarse_axis_offsets(code[a][d], shapes_f[a][d], shapes_c[a][d], code[b][d], shapes_f[b][d], shapes_c[b][d],
                                   o[d]) for d in range(3)]
        for d in range(3):
            # linear P and 2x coarsening: |o| <= 2 gives |J - I| <= 2 (I - 2 <= (i + o - 1) / 2 with i >= 2 I - 1, ...)
            if abs(o[d]) <= 2:
                assert all(abs(v) <= 2 for v in per[d]), (a, b, o, d, per[d])
        for v0 in per[0]:
            for v1 in per[1]:
                for v2 in per[2]:
                    out.add((a, b, (v0, v1, v2)))
    return sorted(out)


def chebyshev_weights(n, lo, hi):
    mid, half = 0.5 * (hi + lo), 0.5 * (hi - lo)
    return [1.0 / (mid - half * math.cos(math.pi * (2 * k + 1) / (2 * n))) for k in range(n)]


class NormalGMG:
    """V-cycle preconditioner for the damped normal equations A = M^T M + damp^2 I + dampdiag^2 diag (reference order,
    linsolver.py:19-23) of a Newton system whose unknowns are all grid `Field`s -- any number, any loc, 1-3 dimensions,
    stencil blocks only.  The reference gives such systems to AMG on the normal equations + CG (linsolver.py:61-72).

      fine level     A assembled from the stencil blocks, one gather launch per (block pair, offset) (odil_bmg_assemble)
      coarse levels  Galerkin products P^T A P, one launch per level (odil_bmg_galerkin); P per field and axis by loc
                     (cells: linear 3/4, 1/4; nodes: coarse node on every second fine node, linear)
      sweeps         Chebyshev-weighted point Jacobi over all fields, one launch each (odil_bmg_apply mode 2 / 3)
      transfers      all fields in one launch (odil_bmg_transfer)
      coarsest       a dense pseudo-inverse applied by odil_lincomb: from np.linalg.eigh on the host (coarse="host", the
                     default) or from a blocked Cholesky on the device (coarse="device": odil_bmg_coarse_dense /
                     odil_bmg_coarse_chol, nothing read back)

    The cycle starts from zero and its post-sweeps repeat the pre-sweeps' weights in reverse order: the preconditioner
    is symmetric (positive definite where A is), as the outer CG needs.  Build with `NormalGMG.create`, which returns
    None (after a log line) when there are more than MAX_FIELDS fields or the hierarchy cannot reach a small enough
    coarsest level."""

    # sweeps before and after the coarse correction, Chebyshev interval [hi / smooth_ratio, hi] (darcy with curl closure,
    # CG iterations to 1e-8 at 512^2 / 64^3: nu = 2 on [hi / 4, hi] 50 / 51, nu = 3 on [hi / 10, hi] 32 / 36, nu = 4 on
    # [hi / 16, hi] 25 / 28 and the shortest solve; kernel log)
    nu = 4
    smooth_ratio = 16.0

    @classmethod
    def create(cls, op, damp=0.0, dampdiag=0.0, coarse="host"):
        from .util import printlog

        pat = normal_pattern(op)
        if pat is None:
            return None
        if len(pat[1]) > MAX_FIELDS:
            printlog("odil_amd: multigrid on the normal equations: {} fields, the kernels take at most {}; "
                     "using CG on the normal equations".format(len(pat[1]), MAX_FIELDS))
            return None
        plan = plan_levels(op.domain.cshape, [op.key_to_field[k].loc for k in pat[1]])
        if plan is None:
            printlog("odil_amd: multigrid on the normal equations: the extents {} do not coarsen to {} unknowns; "
                     "using CG on the normal equations".format(tuple(op.domain.cshape), COARSEST_MAX_UNKNOWNS))
            return None
        return cls(op, pat, plan, damp, dampdiag, coarse=coarse)

    def __init__(self, op, pattern, plan, damp=0.0, dampdiag=0.0, coarse="host"):
        if coarse not in ("host", "device"):
            raise ValueError("NormalGMG: coarse must be 'host' or 'device', got {!r}".format(coarse))
        self.coarse = coarse
        terms, self.keys, shape0 = pattern
        self.shapes, self.codes = plan
        assert [tuple(s) for s in self.shapes[0]] == [tuple(s) for s in shape0]
        self.dtype, self.device = op.dtype, op.device
        self.nf = len(self.keys)
        self.nlvl = len(self.shapes)
        self.ndim = op.domain.ndim
        dev, dt = self.device, self.dtype
        # --- finest level: A = M^T M, terms summed in the order of op.blocks
        fine = dict()
        sizes = [math.prod(s) for s in self.shapes[0]]
        for a, b, o, b1, b2, rmap, rshape in terms:
            arr = fine.get((a, b, o))
            if arr is None:
                arr = fine[(a, b, o)] = torch.zeros(sizes[a], dtype=dt, device=dev)
            rm = torch.as_tensor(rmap, device=dev)
            ops.bmg_assemble(b1[4][0].reshape(-1).contiguous(), b2[4][0].reshape(-1).contiguous(), rm, self.shapes[0][a],
                             rshape, arr)
        for a in range(self.nf):
            if (a, a, (0, 0, 0)) not in fine:
                fine[(a, a, (0, 0, 0))] = torch.zeros(sizes[a], dtype=dt, device=dev)
        if damp or dampdiag:
            # reference linsolver.py:19-23 (as cg_normal): A_ii -> (A_ii + damp^2) (1 + dampdiag^2)
            for a in range(self.nf):
                d = fine[(a, a, (0, 0, 0))]
                d.add_(float(damp) ** 2).mul_(1.0 + float(dampdiag) ** 2)
        entries = sorted(fine)
        self.entries, self.starts, self.coef, self.table, self.desc, self.offs = [], [], [], [], [], []
        self._pack(0, entries, [fine[e] for e in entries])
        del fine
        # --- coarse levels
        self.code_arrays = [(ctypes_int * (3 * self.nf))(*[c for cf in code for c in cf]) for code in self.codes]
        for lvl in range(1, self.nlvl):
            centries = coarse_pattern(self.entries[lvl - 1], self.shapes[lvl - 1], self.shapes[lvl], self.codes[lvl - 1])
            self._pack(lvl, centries, None)
            ops.bmg_galerkin(self.desc[lvl - 1], self.desc[lvl], self.code_arrays[lvl - 1], self.coef[lvl - 1],
                             self.table[lvl - 1], self.table[lvl], len(centries), self.coef[lvl])
        # --- smoothing: Jacobi on D^-1 A, Chebyshev weights on [hi / smooth_ratio, hi], hi a Gershgorin bound (one read-back
        # per level at set-up; an upper bound keeps every sweep polynomial below 1 in modulus on the spectrum: B stays SPD)
        self.dinv, self.weights = [], []
        for lvl in range(self.nlvl):
            diag = torch.empty(self.offs[lvl][-1], dtype=dt, device=dev)
            rowabs = torch.zeros(self.offs[lvl][-1], dtype=dt, device=dev)
            for (a, b, o), start in zip(self.entries[lvl], self.starts[lvl]):
                n = self.offs[lvl][a + 1] - self.offs[lvl][a]
                seg = self.coef[lvl][start:start + n]
                rowabs[self.offs[lvl][a]:self.offs[lvl][a + 1]] += seg.abs()
                if a == b and o == (0, 0, 0):
                    diag[self.offs[lvl][a]:self.offs[lvl][a + 1]] = seg
            dinv = torch.where(diag > 0, 1.0 / torch.where(diag > 0, diag, torch.ones_like(diag)), torch.zeros_like(diag))
            hi = float((rowabs * dinv).max())
            self.dinv.append(dinv)
            self.weights.append(chebyshev_weights(self.nu, hi / self.smooth_ratio, hi))
        # --- coarsest: dense pseudo-inverse (at most COARSEST_MAX_UNKNOWNS unknowns)
        self.coarse_drops = None
        self.coarse_inv = self._coarse_inverse() if coarse == "host" else self._coarse_inverse_device()
        n = [self.offs[l][-1] for l in range(self.nlvl)]
        self.x = [torch.zeros(v, dtype=dt, device=dev) for v in n]
        self.y = [torch.zeros(v, dtype=dt, device=dev) for v in n]
        self.r = [torch.zeros(v, dtype=dt, device=dev) for v in n]
        self.b = [None] + [torch.zeros(v, dtype=dt, device=dev) for v in n[1:]]
        self.method = "gmg-normal ({} field{}, {} levels)".format(self.nf, "s" if self.nf > 1 else "", self.nlvl)

    def _pack(self, lvl, entries, arrays):
        sizes = [math.prod(s) for s in self.shapes[lvl]]
        starts, ebeg, pos = [], [0] * (self.nf + 1), 0
        rows = []
        for e, (a, b, o) in enumerate(entries):
            starts.append(pos)
            rows.append([a, b, o[0], o[1], o[2], pos, 0, 0])
            pos += sizes[a]
            ebeg[a + 1] = e + 1
        for a in range(self.nf):
            ebeg[a + 1] = max(ebeg[a + 1], ebeg[a])
        assert [r[0] for r in rows] == sorted(r[0] for r in rows)
        coef = torch.empty(pos, dtype=self.dtype, device=self.device) if arrays is None else torch.cat(arrays)
        desc, offs = level_desc(self.shapes[lvl], ebeg)
        self.entries.append(list(entries))
        self.starts.append(starts)
        self.coef.append(coef)
        self.table.append(torch.tensor(rows, dtype=torch.int64, device=self.device).reshape(-1))
        self.desc.append(desc)
        self.offs.append(offs)

    def dense(self, lvl):
        """The level's matrix, dense on the host (float64; tests and the coarsest level)."""
        n = self.offs[lvl][-1]
        amat = np.zeros((n, n))
        coef = self.coef[lvl].double().cpu().numpy()
        for (a, b, o), start in zip(self.entries[lvl], self.starts[lvl]):
            sa, sb = self.shapes[lvl][a], self.shapes[lvl][b]
            q = np.indices(sa).reshape(3, -1)
            t = q + np.array(o)[:, None]
            ok = np.all((t >= 0) & (t < np.array(sb)[:, None]), axis=0)
            rows = self.offs[lvl][a] + np.ravel_multi_index(q[:, ok], sa)
            cols = self.offs[lvl][b] + np.ravel_multi_index(t[:, ok], sb)
            np.add.at(amat, (rows, cols), coef[start:start + math.prod(sa)][ok])
        return amat

    def _coarse_inverse(self):
        amat = self.dense(self.nlvl - 1)
        amat = 0.5 * (amat + amat.T)
        w, v = np.linalg.eigh(amat)
        keep = w > 1e-13 * max(float(np.abs(w).max()), 1e-300)
        inv = (v[:, keep] / w[keep]) @ v[:, keep].T
        return torch.as_tensor(inv, dtype=self.dtype).to(self.device).contiguous()

    def _coarse_inverse_device(self):
        """The coarsest level's generalised inverse from a blocked Cholesky on the device (csrc/coarse_chol.hip), float64
        whatever the level's precision.  A pivot <= 1e-13 max_i A_ii (the host route's eigenvalue cut) drops its row and
        column: B = E_S A_SS^-1 E_S^T over the kept pivots S.  B is symmetric positive semidefinite, so the cycle stays
        symmetric and positive semidefinite.  The outer CG's right-hand side M^T r lies in the range of A, so do its
        residuals, and so do their restrictions on a coarse null vector v_c that prolongs to a null vector of A (a
        constant pressure prolongs to a constant: (P v_c)^T r = 0).  There A B b = b: for a one-dimensional nullspace
        v with a dropped pivot d (v_d != 0, A_SS nonsingular), A_dS A_SS^-1 b_S = -v_S^T b_S / v_d = b_d as v^T b = 0.  self.coarse_drops: the dropped pivots per panel
        (device; read back only by `dropped_pivots`)."""
        lvl = self.nlvl - 1
        coef = self.coef[lvl] if self.coef[lvl].dtype == torch.float64 else self.coef[lvl].double()
        inv, self.coarse_drops = ops.bmg_coarse_inverse(coef, self.table[lvl], self.desc[lvl], self.offs[lvl][-1])
        return inv if self.dtype == torch.float64 else inv.to(self.dtype)

    def dropped_pivots(self):
        """Pivots the device factorisation of the coarsest level dropped (one read-back); None for coarse="host"."""
        return None if self.coarse_drops is None else int(self.coarse_drops.sum())

    def apply(self, lvl, x, out=None):
        """out = A_lvl x."""
        out = torch.empty_like(x) if out is None else out
        return ops.bmg_apply(self.coef[lvl], self.table[lvl], self.desc[lvl], x, out, mode=0)

    def restrict(self, lvl, fine, out):
        return ops.bmg_restrict(self.desc[lvl], self.desc[lvl + 1], self.code_arrays[lvl], fine, out)

    def prolong_add(self, lvl, coarse, x):
        return ops.bmg_prolong_add(self.desc[lvl], self.desc[lvl + 1], self.code_arrays[lvl], coarse, x, x)

    def _sweeps(self, lvl, x, b, weights, zero):
        """Jacobi sweeps x' = x + w D^-1 (b - A x); the iterate ping-pongs between x and the level's spare buffer.
        zero: the iterate is the zero vector (x only a buffer).  Returns the tensor holding the result."""
        cur, spare = x, self.y[lvl] if x is not self.y[lvl] else self.x[lvl]
        for k, w in enumerate(weights):
            if zero and k == 0:
                ops.bmg_apply(None, None, self.desc[lvl], None, cur, b=b, dinv=self.dinv[lvl], mode=3, omega=w)
                continue
            ops.bmg_apply(self.coef[lvl], self.table[lvl], self.desc[lvl], cur, spare, b=b, dinv=self.dinv[lvl], mode=2,
                          omega=w)
            cur, spare = spare, cur
        return cur

    def _cycle(self, lvl, b):
        if lvl == self.nlvl - 1:
            x = self.x[lvl]
            return ops.lincomb(x, 0.0, self.coarse_inv, b)
        w = self.weights[lvl]
        x = self._sweeps(lvl, self.x[lvl], b, w, zero=True)
        r = ops.bmg_apply(self.coef[lvl], self.table[lvl], self.desc[lvl], x, self.r[lvl], b=b, mode=1)
        bc = self.restrict(lvl, r, self.b[lvl + 1])
        xc = self._cycle(lvl + 1, bc)
        self.prolong_add(lvl, xc, x)
        return self._sweeps(lvl, x, b, list(reversed(w)), zero=False)

    def precondition(self, r, out=None):
        """z = B r, B one V-cycle from zero (symmetric; no host synchronisation)."""
        z = self._cycle(0, r.contiguous())
        if out is None:
            return z.clone()
        out.copy_(z)
        return out
