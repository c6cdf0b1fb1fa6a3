"""Quasi-Newton and Newton drivers of the slab-decomposed Poisson path (no reference
counterpart: the reference is single-device).  The optimizers are the single-GPU ones -- `optimizer.lbfgsb_minimize`
(the restatement of what the reference calls, reference src/odil/optimizer.py:54-117) and the conjugate-gradient solve of
the Newton step's normal equations (reference src/odil/linsolver.py:17-23, util.py:152-187) -- on vectors that hold ONE
RANK's share of the unknowns:

  * evaluations run the slab kernels of `slab.SlabPoissonAdam` (halo exchanges with the two neighbours, RCCL send / receive);
  * every reduction is formed from the ranks' partial results: the probes of an L-BFGS iteration (loss, <g, d>, <d, d>,
    max |g|) travel as ONE all-gather of eight numbers, the products of the whole (s, y) history with the new vectors
    (the rows of S^T Y, S^T S, Y^T Y of the compact representation and S^T g, Y^T g of the next direction) as ONE
    all-gather of 3 x 2m numbers -- two collectives per iteration instead of 2m sequential dot products; CG: two
    scalar reductions per iteration.  The combined values are the same bits on every rank (sums over the gathered rows
    in rank order), so the ranks take the same branches of the line search without further agreement.

`ThreadComm` runs several ranks as threads of one process (one GPU, or none with the CPU doubles of the tests): the
drivers here are ordinary loops with blocking collectives, not generators.
"""

import threading

import numpy as np
import torch

from . import gmg
from . import ops as hip_ops
from . import slab
from .linsolver import cycle_budget, cycles_accepted
from .optimizer import LbfgsVectors, lbfgsb_minimize


def drive(gen, comm):
    """Runs a generator of the slab path (yields (kind, send_lo, send_hi) at its exchanges) to its end over `comm`."""
    try:
        msg = next(gen)
        while True:
            msg = gen.send(comm.exchange(*msg))
    except StopIteration:
        pass


class ThreadComm:
    """The exchanges of `slab.TorchDistComm` between ranks that are THREADS of one process (tests; one GPU).  A rank
    computes only while it holds the shared token, so the launches of two ranks never interleave (the kernels' shared
    reduction workspaces assume one caller at a time); it hands the token over while it waits at an exchange."""

    class Shared:
        def __init__(self, world):
            self.world = world
            self.barrier = threading.Barrier(world)
            self.token = threading.Lock()
            self.slots = [None] * world

    def __init__(self, rank, shared):
        self.rank, self.world, self.sh = rank, shared.world, shared

    def __enter__(self):
        self.sh.token.acquire()
        return self

    def __exit__(self, *exc):
        self.sh.token.release()
        if exc[0] is not None:
            self.sh.barrier.abort()  # the other ranks must not wait for one that died
        return False

    def _wait(self):
        """The barrier, with the token handed over meanwhile (and held again afterwards even when another rank died and
        the barrier broke: __exit__ releases it)."""
        self.sh.token.release()
        try:
            self.sh.barrier.wait()
        finally:
            self.sh.token.acquire()

    def exchange(self, kind, a, b):
        sh, r, P = self.sh, self.rank, self.world
        if kind == "wait":
            return a
        sh.slots[r] = (a, b)
        self._wait()
        try:
            clone = lambda t: None if t is None else t.clone()
            if kind == "sum":
                total = sh.slots[0][0].clone()
                for i in range(1, P):
                    total = total + sh.slots[i][0]
                return total
            if kind == "gather":
                return torch.stack([sh.slots[i][0] for i in range(P)])
            if kind == "wrap":
                lo = clone(sh.slots[P - 1][1]) if r == 0 else None
                hi = clone(sh.slots[0][0]) if r == P - 1 else None
                return lo, hi
            # "halo" / "post": what the lower neighbour sent up, what the upper one sent down
            return (clone(sh.slots[r - 1][1]) if r > 0 else None, clone(sh.slots[r + 1][0]) if r + 1 < P else None)
        finally:
            self._wait()  # nobody overwrites its slot before everybody has read


def run_threads(world, body):
    """body(rank, comm) -> result on `world` threads joined by a ThreadComm; returns the results in rank order."""
    shared = ThreadComm.Shared(world)
    results, errors = [None] * world, []

    def work(rank):
        try:
            with ThreadComm(rank, shared) as comm:
                results[rank] = body(rank, comm)
        except BaseException as e:  # noqa: BLE001 (re-raised below, on the caller's thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        first = [e for e in errors if not isinstance(e, threading.BrokenBarrierError)] or errors
        raise first[0]
    return results


class SlabLbfgsVectors(LbfgsVectors):
    """`optimizer.LbfgsVectors` over one rank's share of the unknowns: the reductions are combined over the ranks before
    the host reads them (one all-gather each; the sum / max over its rows is formed in rank order on every rank)."""

    def __init__(self, n, m, device, comm):
        super().__init__(n, m, device)
        self.comm = comm

    def reduce_probes(self, scal):
        rows = self.comm.exchange("gather", scal, None)  # (world, 8): dtd, gd_old, -, gd, gg, gmax, f, -
        out = rows.sum(dim=0)
        out[5] = rows[:, 5].max()
        return out

    def reduce_sums(self, t):
        return self.comm.exchange("gather", t, None).sum(dim=0)


class SlabPoissonLbfgs(slab.SlabPoissonAdam):
    """One rank of the slab-decomposed Poisson multigrid problem under L-BFGS-B (3-D, all cell-centred): the unknown
    vector is the undivided one restricted to this rank's planes, level after level."""

    def __init__(self, N, rank, world, dtype=torch.float64, device=None, rhs_global=None):
        super().__init__(N, rank, world, dtype=dtype, device=device, rhs_global=rhs_global, moments=False)
        self.nfev = 0

    def minimize(self, comm, maxiter, m=50, maxls=50, pgtol=1e-16, factr=0.0, callback=None, vectors=None):
        """-> the dict of `lbfgsb_minimize` (task, nit, funcalls, f = GLOBAL loss); the owned planes of self.w hold the
        result.  `vectors`: the vector backend (tests hand in a CPU double)."""
        n = self.n_unknowns_local
        vec = vectors or SlabLbfgsVectors(n, m, self.device, comm)
        x = self.pack_owned(self.w)
        gflat = torch.empty(n, dtype=torch.float64, device=self.device)

        def fg(xflat):
            self.unpack_owned(xflat)
            drive(self.loss_grad_gen(), comm)
            self.nfev += 1
            return self.loss_part.to(torch.float64), self.pack_owned(self.gw, out=gflat)

        res = lbfgsb_minimize(x, fg, vec, maxiter, m=m, maxls=maxls, pgtol=pgtol, factr=factr, callback=callback)
        self.unpack_owned(x)
        return res


def _rank_sum(comm, part):
    """The sum over the ranks of one number per rank: ONE all-gather, added up in rank order on every rank (the same bits
    everywhere, so the ranks take the same branches without further agreement)."""
    return float(comm.exchange("gather", part.to(torch.float64).reshape(1), None).sum())


def _halo_planes(comm, a, lv, planes):
    """`planes` boundary planes of `a` ([..., z, y, x]: one array or a stack of arrays) into the neighbours' ghost planes
    nearest the interface."""
    lo = a[..., lv.g_lo: lv.g_lo + planes, :, :].contiguous() if lv.g_lo else None
    hi = a[..., lv.g_lo + lv.nz - planes: lv.g_lo + lv.nz, :, :].contiguous() if lv.g_hi else None
    recv_lo, recv_hi = comm.exchange("halo", lo, hi)
    if recv_lo is not None:
        a[..., lv.g_lo - planes: lv.g_lo, :, :].copy_(recv_lo.view(lo.shape))
    if recv_hi is not None:
        a[..., lv.g_lo + lv.nz: lv.g_lo + lv.nz + planes, :, :].copy_(recv_hi.view(hi.shape))


class SlabPoissonNewtonCG:
    """One rank of a matrix-free Newton step of the slab-decomposed Poisson problem WITHOUT the multigrid decomposition
    (the reference's `linearize` refuses multigrid unknowns, reference core.py:1208-1209): the step solves the normal
    equations (M^T M + damp^2) dx = -M^T f of the linearisation (reference linsolver.py:17-23) by conjugate gradients;
    M is the Laplacian stencil with the wall rows (its coefficients are the reference's `eval_operator_grad` arrays, SURVEY
    A13), applied by the residual kernel with a zero right-hand side, M^T by the stencil-adjoint kernel.  Per CG iteration:
    one plane of p and one plane of M p to each neighbour (the same halo pattern as an epoch), two scalar reductions."""

    def __init__(self, N, rank, world, dtype=torch.float64, device=None, rhs_global=None, nz=None):
        """The box (world * nz, N, N) with spacing 1 / N, nz (default N) planes per rank."""
        self.ops = hip_ops
        self.N, self.rank, self.world, self.dtype, self.device = N, rank, world, dtype, device
        npdt = np.float64 if dtype == torch.float64 else np.float32
        nz = nz or N
        self.lv = slab.SlabLevel(nz, N, N, rank, world)
        self.h2 = [npdt(1.0 / N) ** 2] * 3
        self.global_cells = world * nz * N * N
        mk = lambda: torch.zeros(self.lv.shape, dtype=dtype, device=device)
        self.u, self.f, self.p, self.q, self.r, self.z = mk(), mk(), mk(), mk(), mk(), mk()
        self.zero = mk()
        self.part = torch.zeros((), dtype=dtype, device=device)
        lv = self.lv
        if rhs_global is not None:
            lo = rank * nz - lv.g_lo
            self.rhs = rhs_global[lo: lo + lv.shape[0]].to(device=device, dtype=dtype).contiguous()
        else:
            assert nz == N, "the built-in reference solution is that of the cubic slabs"
            ref_u = slab.hat_reference_slab(lv, N, rank, world, dtype, device)
            self.rhs, _ = self.ops.poisson_residual(ref_u, torch.zeros_like(ref_u), self.h2)
        self.status = dict()

    def owned(self, a):
        return self.lv.owned(a)

    def _dot(self, comm, a, b):
        return _rank_sum(comm, (self.owned(a).to(torch.float64) * self.owned(b).to(torch.float64)).sum())

    def residual(self, comm, u, out):
        """out = f(u) = Lap(u) - rhs on the owned planes; -> global mean of its squares."""
        _halo_planes(comm, u, self.lv, 1)
        lv = self.lv
        self.ops.poisson_residual(u, self.rhs, self.h2, fu=out, loss=self.part, zrange=(lv.g_lo, lv.g_lo + lv.nz),
                                  denom=self.global_cells)
        return _rank_sum(comm, self.part)

    def normal_apply(self, comm, p, out, damp2=0.0):
        """out = M^T M p + damp2 p on the owned planes (ghost planes of p and of M p refreshed on the way)."""
        _halo_planes(comm, p, self.lv, 1)
        self.ops.poisson_residual(p, self.zero, self.h2, fu=self.q, loss=self.part)
        _halo_planes(comm, self.q, self.lv, 1)
        self.ops.poisson_adjoint(self.q, self.h2, 1.0, out=out)
        if damp2:
            out.add_(p, alpha=damp2)

    def step(self, comm, maxiter=100, tol=1e-10, damp=0.0):
        """One Newton step u <- u + dx; -> (loss before, loss after).  self.status: CG iterations and relative residual."""
        loss0 = self.residual(comm, self.u, self.f)
        # b = -M^T f
        _halo_planes(comm, self.f, self.lv, 1)
        b = self.z
        self.ops.poisson_adjoint(self.f, self.h2, -1.0, out=b)
        dx = torch.zeros_like(self.u)
        r, p, ap = self.r, self.p, torch.zeros_like(self.u)
        r.copy_(b)
        p.copy_(b)
        rr = self._dot(comm, r, r)
        bb, it = rr, 0
        while it < maxiter and rr > tol * tol * bb and rr > 0.0:
            self.normal_apply(comm, p, ap, damp * damp)
            alpha = rr / self._dot(comm, p, ap)
            self.owned(dx).add_(self.owned(p), alpha=alpha)
            self.owned(r).add_(self.owned(ap), alpha=-alpha)
            rr_new = self._dot(comm, r, r)
            beta = rr_new / rr
            self.owned(p).mul_(beta).add_(self.owned(r))
            rr = rr_new
            it += 1
        self.owned(self.u).add_(self.owned(dx))
        loss1 = self.residual(comm, self.u, self.f)
        self.status = dict(niter=it, residual=float(np.sqrt(rr / bb)) if bb > 0 else 0.0)
        return loss0, loss1


class SlabVCycle:
    """GEOMETRIC MULTIGRID on a slab-decomposed 3-D grid: the cycle that `SlabPoissonNewtonGMG` and `SlabStencilGMG` below
    share.  The global grid (world nz, ny, nx) is cut along axis 0, whose two ENDS are walls.

    Levels: the box is coarsened by 2 along every axis while every rank keeps >= 2 planes and the cross-section >= 4
    cells; level arrays are ghost-extended like the epochs' (`slab.SlabLevel`, G = 2 planes per interior interface).  One
    V(nu, nu) cycle per level, everything with the unmodified single-GPU kernels on the extended arrays (an array end that
    is a ghost plane is treated as a wall or wrapped around by the kernel: only the outer ghost planes see that):
      * two planes of x to each neighbour, then TWO Chebyshev-weighted Jacobi sweeps (the first leaves owned + inner ghost
        planes valid, the second the owned planes; as ONE pass on large levels);
      * one plane of x, the residual on the owned planes (its squared norm summed over the ranks by one all-gather),
        full-weighting restriction of the owned planes (pairs of owned planes: no exchange), one plane of the coarse
        right-hand side to each neighbour;
      * the coarse correction; one plane of it to each neighbour, then x += P x_c by the multigrid decomposition's
        prolongation on the ghost-extended coarse array (`SlabLevel.inner`: exact on owned + inner ghost planes);
      * two planes of x, two sweeps.
    Five exchanges per level and cycle, 1 - 2 planes each (512^2 f64 planes: 2 - 4 MB at the finest level, halved twice per
    level).  Below the last slab level the problem is AGGLOMERATED: the coarse right-hand side is all-gathered
    (a few thousand numbers), every rank runs the remaining cycle on the whole coarse box and keeps its planes -- the same
    bits on every rank, no further exchange.

    THE OPERATOR of a level is the subclass's.  `self.mc[l]` (slab levels) and `self.agg[k]` (levels of the agglomerated box)
    hold whatever its kernels take as level data `c`; the cycle never looks inside.  A subclass provides
      sweep(c, src, b, w, out), sweep_pair(c, src, b, w1, w2, out), pair_supported(x)
      level_residual(c, x, b, out=None, lv=None)   the residual; lv: a slab level (only its owned planes matter)
      rank_norm(r, lv)                             this rank's share of |r|^2 after level_residual(..., r, lv)
      residual_restrict(c, x, b, out, lv), fused_supported(x)    residual + restriction in one pass, the share in self.part
      rhs_sign              the coarse right-hand side is rhs_sign R (what `level_residual` returns)
      coarsen(c)            level data of the next level of a WHOLE box
      box_solver(c)         the single-GPU solver that cycles the agglomerated box
      invert(amat)          the dense solve at the bottom of a stand-in's recursion
      top2(l)               whether level l's coarse correction takes a second cycle
      method                the name `status` reports
    and self.ops, rank, world, dtype, device, nu, pair_min_cells."""

    def _plan(self, first, agg_cells):
        """The slab levels below `first` and the shape of the agglomerated box.  agg_cells: a level is a SLAB level only
        while a rank holds more cells of it than this -- an exchange costs ~65 us of host time whatever its size
        (`profiles/r06_rccl_selfloop_sweep.txt`), four of them per level and cycle, and a level of 32^3 cells per rank is
        sooner solved redundantly on the whole agglomerated box (0: down to two planes per rank)."""
        # The library's own kernels, or a stand-in `ops` (the host tests)?  With its own the cycle is the single-GPU one's:
        # sweeps in pairs, the residual restricted in the pass that forms it, a zero iterate that is never read, the
        # agglomerated box cycled by `gmg`; a stand-in keeps the plain launches and the plain recursion of `_box_cycle`.
        self.native = getattr(self.ops, "__name__", "") == "odil_amd.ops"
        self.mlv = [first]
        shape = (first.nz, first.ny, first.nx)
        # (cross-sections of >= 4 cells on every slab level, so that the agglomerated box below the last one still has two)
        while (all(s % 2 == 0 for s in shape) and shape[0] // 2 >= 2 and min(shape[1], shape[2]) // 2 >= 4
               and int(np.prod(shape)) // 8 > agg_cells):
            shape = tuple(s // 2 for s in shape)
            self.mlv.append(slab.SlabLevel(shape[0], shape[1], shape[2], self.rank, self.world))
        # the agglomerated box below the last slab level (None when that level cannot be coarsened at all)
        last = self.mlv[-1]
        self.agg_shape = None
        if last.nz % 2 == 0 and last.ny % 2 == 0 and last.nx % 2 == 0 and min(last.ny, last.nx) >= 4:
            self.agg_shape = (self.world * last.nz // 2, last.ny // 2, last.nx // 2)

    def _finish_setup(self, box):
        """The work arrays of the slab levels, and the levels of the agglomerated box from its level data `box` (None: no
        box)."""
        mk = lambda lv: torch.zeros(lv.shape, dtype=self.dtype, device=self.device)
        self.mx = [None] + [mk(lv) for lv in self.mlv[1:]]
        self.mb = [None] + [mk(lv) for lv in self.mlv[1:]]
        self.spare = [mk(lv) for lv in self.mlv]
        self.res = [mk(lv) for lv in self.mlv]
        self.part = torch.zeros((), dtype=self.dtype, device=self.device)
        self.agg = self.agg_gmg = self._agg_part = self._box_inv = None
        if box is not None:
            self.agg, shape = [box], self.agg_shape
            while all(v % 2 == 0 and v // 2 >= 2 for v in shape) and int(np.prod(shape)) > 512:
                self.agg.append(self.coarsen(self.agg[-1]))
                shape = tuple(v // 2 for v in shape)
            if self.native and min(self.agg_shape) >= 4:
                self.agg_gmg = self.box_solver(box)  # (its paired sweeps and one-launch coarse tail)

    # ---- the cycle on the slab levels -----------------------------------------------------------------------------------
    def _smooth(self, comm, l, x, b, zero=False):
        """`nu` sweeps, two per exchange of two planes; returns the tensor holding the iterate (owned planes valid).
        zero: x is zero on every rank -- its ghost planes are right as they are, the first exchange is skipped."""
        lv, c, w = self.mlv[l], self.mc[l], gmg.jacobi_weights(3, self.nu)
        for k in range(0, len(w), 2):
            pair = w[k: k + 2]
            first = zero and k == 0
            if not first:
                _halo_planes(comm, x, lv, min(2, lv.nz) if len(pair) == 2 else 1)
            # (native kernels do not read a zero iterate: src = None -- the bits of the same launch on an array of zeros)
            src = None if (first and self.native) else x
            if self.native and len(pair) == 2 and lv.size >= self.pair_min_cells and self.pair_supported(x):
                y = self.spare[l]
                self.sweep_pair(c, src, b, pair[0], pair[1], y)  # (== the two sweeps below, bit for bit)
                self.spare[l], x = x, y
                continue
            for wk in pair:
                y = self.spare[l]
                self.sweep(c, src, b, wk, y)
                self.spare[l], x, src = x, y, y
        return x

    def _vcycle(self, comm, l, x, b, zero=False):
        """One V(nu, nu) cycle on level l of the slab hierarchy: returns the tensor holding the iterate (owned planes)."""
        lv, c = self.mlv[l], self.mc[l]
        x = self._smooth(comm, l, x, b, zero=zero)
        r = self.res[l]
        below = l + 1 < len(self.mlv)
        coarser = below or self.agg_shape is not None
        _halo_planes(comm, x, lv, 1)
        if coarser and self.native and x.shape[0] % 2 == 0 and lv.g_lo % 2 == 0 and self.fused_supported(x):
            # residual and restriction in ONE pass over the ghost-extended arrays (the fine residual is never stored),
            # straight into the coarse right-hand side: its owned planes + one plane per interface, formed from the fine
            # ghost planes, that nobody reads
            if below:
                lc = self.mlv[l + 1]
                target = self.mb[l + 1][lc.g_lo - lv.g_lo // 2: lc.g_lo + lc.nz + lv.g_hi // 2]
            else:
                if self._agg_part is None:
                    self._agg_part = torch.empty(tuple(n // 2 for n in x.shape), dtype=self.dtype, device=self.device)
                target = self._agg_part
            self.residual_restrict(c, x, b, target, lv)
            r = None
        else:
            self.level_residual(c, x, b, r, lv)
        if l == 0:
            # (the coarser levels' residuals belong to THEIR systems, only the finest one is the solve's measure: no
            # collective, no read-back below it)
            self._last_res2 = _rank_sum(comm, self.part if r is None else self.rank_norm(r, lv))
        if coarser:
            xc = self._coarse_correction(comm, l, r)
            y = self.spare[l]
            self.ops.interp_add(xc.contiguous(), "ccc", add=x, out=y)
            self.spare[l] = x
            x = y
        return self._smooth(comm, l, x, b)

    def _restricted(self, r):
        """The coarse right-hand side from a stored residual (the mean of the children, with the operator's sign)."""
        rc = self.ops.restrict_to_coarser(r, "ccc")
        return rc if self.rhs_sign == 1.0 else rc.mul_(self.rhs_sign)

    def _coarse_correction(self, comm, l, r):
        """x_c with A_c x_c ~= the restricted residual of level l (r: the stored residual, owned planes valid; None: the
        fused pass has written the coarse right-hand side); returned on level l + 1's ghost-extended array with owned +
        inner ghost planes valid."""
        lv, twice = self.mlv[l], self.top2(l)
        if l + 1 < len(self.mlv):
            lc = self.mlv[l + 1]
            bc, xc = self.mb[l + 1], self.mx[l + 1]
            if r is not None:
                lc.owned(bc).copy_(self._restricted(lv.owned(r).contiguous()))
            _halo_planes(comm, bc, lc, 1)
            if not self.native:
                xc.zero_()
            xc = self._vcycle(comm, l + 1, xc, bc, zero=True)
            if twice:
                xc = self._vcycle(comm, l + 1, xc, bc)
            self.mx[l + 1] = xc
            _halo_planes(comm, xc, lc, 1)
            return lc.inner(xc)
        # agglomerated: every rank gets the whole coarse right-hand side and solves the whole coarse problem alike
        if r is not None:
            part = self._restricted(lv.owned(r).contiguous())
        else:
            part = self._agg_part[lv.g_lo // 2: lv.g_lo // 2 + lv.nz // 2]
        bc = comm.exchange("gather", part.contiguous(), None).reshape(self.agg_shape).contiguous()
        if self.agg_gmg is not None:
            xc = self.agg_gmg.vcycle(0, torch.zeros_like(bc), bc, zero=True)
            if twice:
                xc = self.agg_gmg.vcycle(0, xc, bc)
        else:
            xc = self._box_cycle(0, torch.zeros_like(bc), bc)
            if twice:
                xc = self._box_cycle(0, xc, bc)
        nzc = lv.nz // 2
        lo = self.rank * nzc - (1 if self.rank > 0 else 0)
        hi = (self.rank + 1) * nzc + (1 if self.rank < self.world - 1 else 0)
        return xc[lo:hi]

    def _box_cycle(self, k, x, b):
        """One V(nu, nu) cycle on level k of the agglomerated box, held whole by this rank, by plain launches (a stand-in
        `ops`; the library's own kernels go through `box_solver`): returns the iterate."""
        c = self.agg[k]
        if k == len(self.agg) - 1:
            if b.numel() > 512:  # (cannot coarsen further: by iteration)
                for _ in range(20):
                    for wk in gmg.jacobi_weights(3, 2):
                        x = self.sweep(c, x, b, wk, torch.empty_like(x))
                return x
            if self._box_inv is None:  # (the residual kernel applied to unit vectors, factorised once)
                n = b.numel()
                eye = torch.eye(n, dtype=self.dtype, device=self.device)
                zero = torch.zeros_like(b)
                cols = [self.level_residual(c, eye[j].view(b.shape).contiguous(), zero).reshape(-1) for j in range(n)]
                amat = -self.rhs_sign * torch.stack(cols, dim=1).cpu().numpy().astype(np.float64)  # column j = A e_j
                self._box_inv = torch.as_tensor(self.invert(amat), dtype=self.dtype).to(self.device)
            return (self._box_inv @ b.reshape(-1)).view(b.shape)
        for wk in gmg.jacobi_weights(3, self.nu):
            x = self.sweep(c, x, b, wk, torch.empty_like(x))
        bc = self._restricted(self.level_residual(c, x, b))
        xc = self._box_cycle(k + 1, torch.zeros_like(bc), bc)
        x = self.ops.interp_add(xc.contiguous(), "ccc", add=x)
        for wk in gmg.jacobi_weights(3, self.nu):
            x = self.sweep(c, x, b, wk, torch.empty_like(x))
        return x

    def _cycles(self, comm, b, tol, maxiter, stall):
        """V-cycles from the zero iterate on A x = b (b: level 0's ghost-extended array, owned planes valid) until
        |residual| <= tol |b| over all ranks; returns the tensor holding x and leaves self.status: niter, residual,
        converged, stagnated, method.  stall=True: also stop where the cycles stopped gaining -- from the fourth cycle on, a
        residual above 0.98 of the previous cycle's (the rule of gmg.StencilGMG.solve, counted in cycles done) -- and say
        so in status["stagnated"] (below 1: the rounding floor of the working precision, not divergence)."""
        lv = self.mlv[0]
        _halo_planes(comm, b, lv, 1)
        bb = _rank_sum(comm, (lv.owned(b).to(torch.float64) ** 2).sum())
        x = torch.zeros_like(b)
        it, rel, stagnated = 0, 1.0, False
        while it < maxiter:
            x = self._vcycle(comm, 0, x, b)
            it += 1
            # (the residual a cycle forms on its way down belongs to its pre-smoothed iterate: a cheap, slightly
            # pessimistic convergence test that costs no pass of its own)
            prev, rel = rel, float(np.sqrt(self._last_res2 / bb)) if bb > 0 else 0.0
            if rel <= tol:
                break
            if stall and it > 3 and rel >= 0.98 * prev:
                stagnated = rel == rel and rel < 1.0  # (not: diverging; the same numbers, so the same branch, on every rank)
                break
        self.status = dict(niter=it, residual=rel, converged=rel <= tol, stagnated=stagnated, method="{} ({} slab levels{})".format(
            self.method, len(self.mlv), " + agglomerated {}".format(self.agg_shape) if self.agg_shape else ""))
        return x


class SlabPoissonNewtonGMG(SlabVCycle, SlabPoissonNewtonCG):
    """The Newton step of the slab-decomposed Poisson problem solved by `SlabVCycle` -- the slab form of `gmg.PoissonGMG`
    ("Newton: matrix-free M / M^T apply = same halo pattern"; the reference's Newton driver,
    src/odil/util.py:152-187, solves M^T M delta = -M^T f with SuperLU, linsolver.py:17-26; for the square nonsingular
    Laplacian M delta = -f has the same solution).  `SlabPoissonNewtonCG` above is unpreconditioned CG on the normal
    equations: O(N) iterations; this one needs ~12 cycles at any size.  Level data: the squared spacings (the same stencil
    rediscretised); the residual is A x - b, its norm over the rank's own planes formed by the kernels."""

    rhs_sign = -1.0
    method = "slab gmg-vcycle"

    def __init__(self, N, rank, world, dtype=torch.float64, device=None, rhs_global=None, nz=None, nu=2, agg_cells=32**3,
                 pair_min_cells=128**3):
        """agg_cells: see `SlabVCycle._plan`."""
        super().__init__(N, rank, world, dtype=dtype, device=device, rhs_global=rhs_global, nz=nz)
        self.nu, self.pair_min_cells = nu, pair_min_cells
        self._plan(self.lv, agg_cells)
        self.mc = [list(self.h2)]
        for _ in self.mlv[1:]:
            self.mc.append(self.coarsen(self.mc[-1]))
        self._finish_setup(self.coarsen(self.mc[-1]) if self.agg_shape else None)

    def sweep(self, h2, src, b, w, out):
        return self.ops.poisson_jacobi(src, b, h2, w, out=out)

    def sweep_pair(self, h2, src, b, w1, w2, out):
        self.ops.poisson_jacobi2(src, b, h2, w1, w2, out=out)  # (`odil_poisson_jacobi2`)

    def pair_supported(self, x):
        return self.dtype == torch.float64 and self.ops.jacobi2_supported(tuple(x.shape), self.dtype)

    def level_residual(self, h2, x, b, out=None, lv=None):
        """A x - b."""
        return self.ops.poisson_residual(x, b, h2, fu=out, loss=self.part, denom=1.0,
                                         zrange=None if lv is None else (lv.g_lo, lv.g_lo + lv.nz))[0]

    def rank_norm(self, r, lv):
        return self.part

    def residual_restrict(self, h2, x, b, out, lv):
        """(`odil_poisson_residual_restrict_slab` counts the rank's own planes)"""
        self.ops.poisson_residual_restrict(x, b, h2, 0.125 * self.rhs_sign, out, self.part,
                                           zrange=(lv.g_lo, lv.g_lo + lv.nz), denom=1.0)

    def fused_supported(self, x):
        return self.ops.residual_restrict_supported(tuple(x.shape), self.dtype)

    def coarsen(self, h2):
        return [v * 4 for v in h2]

    def box_solver(self, h2):
        return gmg.PoissonGMG(self.agg_shape, h2, self.dtype, self.device)

    invert = staticmethod(gmg.PoissonGMG.invert)

    def top2(self, l):
        return False

    def step(self, comm, maxiter=40, tol=1e-10, damp=0.0):
        """One Newton step u <- u + delta with A delta = -f(u) by V-cycles; -> (loss before, loss after).
        self.status: cycles, relative residual of the linear system, converged."""
        assert not damp, "the multigrid step solves the undamped system"
        loss0 = self.residual(comm, self.u, self.f)
        b = self.z
        b.copy_(self.f).mul_(-1.0)  # owned planes valid; the neighbours' planes of b follow
        x = self._cycles(comm, b, tol, maxiter, stall=False)  # (to tol or maxiter: no stall rule for this step)
        self.owned(self.u).add_(self.owned(x))
        loss1 = self.residual(comm, self.u, self.f)
        return loss0, loss1


class SlabStencilGMG(SlabVCycle):
    """`SlabVCycle` for ANY (2 d + 1)-point operator with variable coefficients -- the slab form of `gmg.StencilGMG` (the
    Newton system M delta = -r of a single-field operator from its Jacobian's coefficient arrays, reference
    src/odil/core.py:1113-1217, linsolver.py:17-26; SURVEY 8 E: "Newton: matrix-free M / M^T apply = same halo pattern").
    The operator has zero coefficients towards the two ends of the cut axis (a periodic cut axis would need the ring
    closure).

    Every rank holds its planes of the 7 coefficient arrays; level data are the ghost-extended coefficient arrays.  Set-up,
    once per solve (the coefficients change with the state): two boundary planes of the seven arrays to each neighbour
    (ONE packed message per level); the coarse operators by `odil_stencil_var_coarsen` on the extended arrays --
    aggregates of 2^3 cells never straddle an interface, the matrix-symmetric split reads the neighbour's coefficient one
    plane into the valid ghosts; for the agglomerated box the coefficient arrays are all-gathered.  The residual is
    b - A x, the coarse right-hand side the mean of its children."""

    rhs_sign = 1.0
    method = "slab variable-coefficient gmg"

    def __init__(self, coeffs, rank, world, ops=None, nu=2, pair_min_cells=128**3, agg_cells=32**3):
        """agg_cells: see `SlabVCycle._plan`."""
        assert coeffs.dim() == 4 and coeffs.shape[0] == 7 and coeffs.is_contiguous()
        self.ops = ops or hip_ops
        self.rank, self.world, self.nu, self.pair_min_cells = rank, world, nu, pair_min_cells
        self.dtype, self.device = coeffs.dtype, coeffs.device
        nz, ny, nx = (int(v) for v in coeffs.shape[1:])
        self._plan(slab.SlabLevel(nz, ny, nx, rank, world), agg_cells)
        self.c_owned = coeffs
        self.mc = None  # ghost-extended coefficient arrays per slab level, built by setup(comm)
        self.status = dict()

    def setup(self, comm):
        """The operators of every level (see the class text); the agglomerated hierarchy below the last slab level."""
        self.mc = []
        for l, lc in enumerate(self.mlv):
            # (level 0: the caller's arrays; below: the coarsened extended arrays of the level above, its owned planes' part)
            cc_all, first = (self.coarsen(self.mc[-1]), self.mlv[l - 1].g_lo // 2) if l else (self.c_owned, 0)
            c = torch.zeros((7,) + lc.shape, dtype=self.dtype, device=self.device)
            c[:, lc.g_lo: lc.g_lo + lc.nz].copy_(cc_all[:, first: first + lc.nz])
            # ghost rows that no neighbour fills (the outer planes of a thin level) keep a unit diagonal: the sweeps divide by it
            if lc.g_lo:
                c[0, : lc.g_lo].fill_(1.0)
            if lc.g_hi:
                c[0, lc.g_lo + lc.nz:].fill_(1.0)
            _halo_planes(comm, c, lc, min(slab.G, lc.nz))
            self.mc.append(c)
        # the agglomerated box: every rank gets the whole coarse operator of the level below the last slab level
        whole = None
        if self.agg_shape is not None:
            last = self.mlv[-1]
            part = self.coarsen(self.mc[-1])[:, last.g_lo // 2: last.g_lo // 2 + last.nz // 2].contiguous()
            rows = comm.exchange("gather", part, None)  # (world, 7, nz / 2, ny / 2, nx / 2)
            whole = torch.cat([rows[r] for r in range(self.world)], dim=1).contiguous()
        self._finish_setup(whole)

    def sweep(self, c, src, b, w, out):
        return self.ops.stencil_var_smooth(c, src, b, w, out=out)

    def sweep_pair(self, c, src, b, w1, w2, out):
        self.ops.stencil_var_smooth2(c, src, b, w1, w2, out=out)  # (`odil_stencil_var_smooth2`)

    def pair_supported(self, x):
        return x.shape[-1] % 2 == 0

    def level_residual(self, c, x, b, out=None, lv=None):
        """b - A x."""
        return self.ops.stencil_var_residual(c, x, b, out=out)

    def rank_norm(self, r, lv):
        return (lv.owned(r).to(torch.float64) ** 2).sum()

    def residual_restrict(self, c, x, b, out, lv):
        self.ops.stencil_var_residual_restrict(c, x, b, 0.125 * self.rhs_sign, out, self.part,
                                               zrange=(lv.g_lo, lv.g_lo + lv.nz), denom=1.0)

    def fused_supported(self, x):
        return x.shape[2] % 2 == 0

    def coarsen(self, c):
        return self.ops.stencil_var_coarsen(c.contiguous())

    def box_solver(self, c):
        return gmg.StencilGMG(c)

    invert = staticmethod(gmg.StencilGMG.invert)

    def top2(self, l):
        """TWO cycles on the first coarse level (a slab level or the agglomerated box) when there is a level below it, as
        gmg.StencilGMG.finish_cycle: the aggregation-built coarse operators are less accurate at the walls than a
        rediscretisation (0.24 -> 0.14 per cycle there)."""
        return l == 0 and len(self.mlv) + len(self.agg or ()) > 2

    def solve(self, comm, b_owned, tol=1e-10, maxiter=40, stall=False):
        """x (owned planes) with A x = b to |b - A x| <= tol |b| over all ranks; self.status and `stall`: `_cycles`."""
        if self.mc is None:
            self.setup(comm)
        lv = self.mlv[0]
        b = torch.zeros(lv.shape, dtype=self.dtype, device=self.device)
        lv.owned(b).copy_(b_owned)
        return lv.owned(self._cycles(comm, b, tol, maxiter, stall)).clone()


class ReplicatedTailVectors(SlabLbfgsVectors):
    """`SlabLbfgsVectors` for a local vector [owned entries | entries EVERY rank holds] (coarse levels agglomerated on
    every rank, network parameters): the tail takes part in every rank's vector algebra -- all ranks then update it alike,
    from the same combined scalars -- but must count ONCE in the reductions: every rank enters its tail products with
    the weight 1 / world (whole-vector product minus (1 - 1 / world) of the tail's, two launches instead of one)."""

    def __init__(self, n, m, device, comm, n_own, world):
        super().__init__(n, m, device, comm)
        self.n_own, self.excess = n_own, 1.0 - 1.0 / world
        self.tail = n > n_own and world > 1
        self.tscal = torch.zeros(8, dtype=torch.float64, device=device)

    def probe_direction(self, d, g):
        super().probe_direction(d, g)
        if self.tail:
            k = self.n_own
            hip_ops.dots3(d[None, k:], [d[k:], g[k:]], out=self.tscal[0:3].view(3, 1))

    def probe_eval(self, f, g, d):
        super().probe_eval(f, g, d)
        if self.tail:
            k = self.n_own
            hip_ops.dots3(g[None, k:], [d[k:], g[k:]], out=self.tscal[3:6].view(3, 1))  # <g, d>, <g, g> of the tail

    def reduce_probes(self, scal):
        if self.tail:
            fixed = scal.clone()
            fixed[0:2] -= self.excess * self.tscal[0:2]
            fixed[3:5] -= self.excess * self.tscal[3:5]
            scal = fixed
        return super().reduce_probes(scal)

    def history_products(self, nphys, bs):
        if nphys == 0 or not self.tail:
            return super().history_products(nphys, bs)
        k = self.n_own
        whole = hip_ops.dots3(self.w[: 2 * nphys], bs)
        tail = hip_ops.dots3(self.w[: 2 * nphys, k:], [b[k:] for b in bs])
        out = self.reduce_sums(whole - self.excess * tail).cpu().numpy()[: len(bs)]
        return out[:, 0::2], out[:, 1::2]

    def dot(self, a, b):
        k = self.n_own
        whole = hip_ops.dots3(a[None], [b])
        if self.tail:
            whole = whole - self.excess * hip_ops.dots3(a[None, k:], [b[k:]])
        return float(self.reduce_sums(whole).cpu().numpy()[0, 0])


class SlabTracedLbfgs:
    """L-BFGS-B for ANY traced operator on the slab decomposition of `slab_traced.SlabTracedAdam` (whose evaluation it
    borrows: `epoch_gen(update=False)`).  The local vector: this rank's owned planes of every level of every field,
    then what every rank holds whole (agglomerated coarse levels, network / `Array` parameters)."""

    def __init__(self, run):
        self.run = run
        self.index = run.layout.local_index(run.device)
        self.n_own, self.n = run.layout.n_owned, run.layout.n_unknowns_local
        self.nfev = 0

    def pack(self, flat, out=None):
        res = flat.index_select(0, self.index).to(torch.float64)
        if out is None:
            return res
        out.copy_(res)
        return out

    def unpack(self, vec, flat):
        flat.index_copy_(0, self.index, vec.to(flat.dtype))

    def local_loss(self):
        """This rank's share of the loss of the last evaluation (the ranks' shares add up to the loss)."""
        run = self.run
        part = run.kern.partial_terms().to(torch.float64).sum()
        for _, value in run.par_terms():  # (counted once: `SlabTracedAdam.par_terms`)
            if value is not None:
                part = part + value.to(torch.float64)
        return part

    def minimize(self, comm, maxiter, m=50, maxls=50, pgtol=1e-16, factr=0.0, callback=None, vectors=None):
        """-> the dict of `lbfgsb_minimize` (f = GLOBAL loss); the unknowns of `self.run` hold the result."""
        run = self.run
        vec = vectors or ReplicatedTailVectors(self.n, m, run.device, comm, self.n_own, run.world)
        x = self.pack(run.x)
        gflat = torch.empty(self.n, dtype=torch.float64, device=run.device)

        def fg(xflat):
            self.unpack(xflat, run.x)
            drive(run.epoch_gen(update=False), comm)
            self.nfev += 1
            return self.local_loss(), self.pack(run.g, out=gflat)

        res = lbfgsb_minimize(x, fg, vec, maxiter, m=m, maxls=maxls, pgtol=pgtol, factr=factr, callback=callback)
        self.unpack(x, run.x)
        run.unknowns_changed()
        return res


def check_slab_newton(args, problem, state, axis=None, world=1):
    """Raises NotImplementedError, with the reason, unless Newton on the slab decomposition covers this run: a 3-D grid cut
    along axis 0, ONE unknown that is a plain cell-centred `Field`, a square (2 d + 1)-point Jacobian (decided from the
    `jac_items` of the generated Jacobian kernel, traced on the host: no GPU, no compiler), no damping, `--linsolver`
    multigrid or direct.  (Walls across the cut axis are checked on the coefficients, by every step: SlabTracedNewton.)"""
    from .core import Field
    from .stencil_codegen import _Codegen
    from .stencil_jit import trace_outputs
    from .stencil_trace import TraceUnsupported

    domain = problem.domain
    if domain.ndim != 3:
        raise NotImplementedError("Newton on the slab decomposition: {}-D grid (3-D only)".format(domain.ndim))
    if axis not in (None, 0):
        raise NotImplementedError("Newton on the slab decomposition: cut along axis {} (axis 0 only)".format(axis))
    fields = list(state.fields.items())
    if len(fields) != 1:
        raise NotImplementedError("Newton on the slab decomposition: {} unknowns ({}; one Field only)".format(
            len(fields), ", ".join(k for k, _ in fields)))
    key, field = fields[0]
    if type(field) is not Field:
        raise NotImplementedError("Newton on the slab decomposition: unknown '{}' is a {} (a plain Field only)".format(
            key, type(field).__name__))
    if field.loc != "ccc":
        raise NotImplementedError("Newton on the slab decomposition: field '{}' at loc '{}' (cell-centred only)".format(
            key, field.loc))
    damp, dampdiag = getattr(args, "linsolver_damp", 0) or 0, getattr(args, "linsolver_dampdiag", 0) or 0
    if damp or dampdiag:
        raise NotImplementedError("Newton on the slab decomposition: damping (linsolver_damp={}, linsolver_dampdiag={})".format(
            damp, dampdiag))
    linsolver = getattr(args, "linsolver", "direct")
    if linsolver not in ("multigrid", "direct"):
        raise NotImplementedError("Newton on the slab decomposition: linsolver '{}' (multigrid, direct)".format(linsolver))
    N = domain.cshape[0]
    if N % world:
        raise NotImplementedError("Newton on the slab decomposition: {} cells on axis 0 over {} ranks".format(N, world))
    try:
        tr, outs, raw, _, G = trace_outputs(problem, state)
        cg = _Codegen(tr, outs, raw, G, state, slab=(0, N // world), jac=True)
        cg.source()
    except TraceUnsupported as e:
        raise NotImplementedError("Newton on the slab decomposition: no generated Jacobian kernel ({})".format(e))
    if len(outs) != 1:
        raise NotImplementedError("Newton on the slab decomposition: {} outputs (a square Jacobian has one)".format(len(outs)))
    want = [(0, 0, 0)] + [tuple(s if j == i else 0 for j in range(3)) for i in range(3) for s in (-1, 1)]
    for _, attr in cg.jac_items:
        if attr is None:
            continue
        rkey, shift, loc = attr[0], tuple(int(v) for v in attr[1]), attr[2]
        norm = tuple(((s + n // 2) % n) - n // 2 for s, n in zip(shift, G))
        if rkey != key or loc != field.loc or norm not in want:
            raise NotImplementedError("Newton on the slab decomposition: the Jacobian reads '{}' at shift {} loc '{}' "
                                      "(a (2 d + 1)-point stencil only)".format(rkey, shift, loc))
    if not any(attr is not None and not any(((s + n // 2) % n) - n // 2 for s, n in zip(attr[1], G))
               for _, attr in cg.jac_items):
        raise NotImplementedError("Newton on the slab decomposition: the Jacobian has no diagonal")


class SlabTracedNewton:
    """Newton (`util.optimize_newton`) on the slab decomposition of `slab_traced.SlabTracedAdam` (whose layout, unknowns and
    exchanges it borrows; its kernels must carry `k_jac`: HipSlabKernels(..., jac=True)), for what `check_slab_newton`
    admits.  One step: the ghost and wrap planes of u, `k_jac` on the owned cells -> the value r and the 7 coefficient
    arrays of M (a view of the kernel's buffer), the walls across the cut ends checked, M d = r solved by `SlabStencilGMG`,
    x <- x - d on the owned planes, and one forward evaluation (the loss of the new state: `run.last_terms`)."""

    def __init__(self, run, linsolver="multigrid", tol=1e-10, maxiter=None):
        self.run = run
        if len(run.entries) != 1 or run.entries[0].kind != "field" or run.axis != 0:
            raise NotImplementedError("Newton on the slab decomposition: one Field cut along axis 0")
        if not getattr(run.kern, "jac_items", None):
            raise RuntimeError("SlabTracedNewton needs slab kernels generated with their Jacobian kernel (jac=True)")
        tol, self.maxiter = cycle_budget(linsolver, tol, maxiter)
        self.tol = max(tol, 50 * float(torch.finfo(run.dtype).eps))  # (the floor of gmg.StencilGMG.solve)
        self.status = dict()
        self._evaluated = False

    def step(self, comm):
        run = self.run
        e = run.entries[0]
        lv = e.levels[0]
        if not self._evaluated:  # (else the evaluation that ended the last step left u and the wrap planes of this state)
            drive(run.evaluate_gen(), comm)
        buf = run.kern.jacobian(run.u, *run.wrap_planes())
        items = [(attr[1], buf[j]) for j, (_, attr) in enumerate(run.kern.jac_items) if attr is not None]
        r = buf[next(j for j, (_, attr) in enumerate(run.kern.jac_items) if attr is None)]
        coeffs = gmg.stencil_coefficients(items, tuple(buf.shape[1:]), period=run.domain.cshape)
        if coeffs is None:
            raise NotImplementedError("Newton on the slab decomposition: the Jacobian is not a (2 d + 1)-point stencil")
        # walls across the cut ends: nothing below the first plane of rank 0 and nothing above the last plane of the last
        # rank may couple (a periodic cut axis needs the ring closure SlabStencilGMG does not have)
        bad = torch.zeros(1, dtype=torch.float64, device=run.device)
        if run.rank == 0:
            bad += (coeffs[1, 0] != 0).sum().to(torch.float64)
        if run.rank == run.world - 1:
            bad += (coeffs[2, -1] != 0).sum().to(torch.float64)
        if float(comm.exchange("gather", bad, None).sum()) > 0:
            raise NotImplementedError("Newton on the slab decomposition: the operator couples across the ends of the cut "
                                      "axis (periodic); walls only")
        solver = SlabStencilGMG(coeffs if coeffs.is_contiguous() else coeffs.contiguous(), run.rank, run.world)
        solver.setup(comm)
        d = solver.solve(comm, r, tol=self.tol, maxiter=self.maxiter, stall=True)
        st = solver.status
        self.status = dict(niter=st["niter"], residual=st["residual"], converged=st["converged"], stagnated=st["stagnated"],
                           method=st["method"])
        if not cycles_accepted(st, bnorm=1.0):  # (the single-GPU rule; this status carries the RELATIVE residual)
            raise RuntimeError("Newton on the slab decomposition: multigrid stopped at relative residual {:.3e} after {} "
                               "cycles (tolerance {:.1e}); the step is not applied".format(st["residual"], st["niter"], self.tol))
        hip_ops.axpy(lv.owned(e.x[0]), d, -1.0)
        run.unknowns_changed()
        drive(run.evaluate_gen(), comm)  # the loss of the new state, and the sources of the next step
        self._evaluated = True
        return self.status
