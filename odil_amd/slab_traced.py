"""Slab decomposition of TRACED operators over the GPUs of one node: any `operator(ctx)` the tracer can
express (odil_amd/stencil_jit.py) -- the tracer-velocity workload BASELINE.json names for 8 GPUs -- with an
Adam loop per rank.  No reference counterpart (the reference is single-device).

Layout.  The grid is cut along ONE domain axis `a` on which every grid field is cell-centred (for the
(t, x, y[, z]) workloads: x; the node-centred time axis stays whole).  Rank r owns n = N_a / P cells of every
multigrid level (every level keeps >= 2 owned cells per rank).  Level arrays are stored ghost-extended along
`a` exactly as in the Poisson slab path (odil_amd/slab.py): G = 2 ghost cells at every interior interface,
none at the two ends of the decomposition, where the prolongation has its wall rule.  All unknowns of a rank
(level arrays of all fields, then replicated network / Array parameters) live in one packed vector.

Per epoch and rank:
  1. ("halo") the first / last OWNED plane of every level array of every field -> the neighbours' inner ghost
     planes, one packed message per neighbour;
  2. u = w_0 + P(w_1 + P(...)) per field with the unmodified single-GPU transfer kernels run on the extended
     arrays: a coarse array with one valid ghost plane gives a fine array whose inner ghost plane is exact
     (the wall formulas only ever reach the outer one, which nobody reads);
  3. ("wrap") `Context.field` rolls PERIODICALLY (reference core.py:962-963): what owned cells of the first
     rank read below the grid is the last rank's last plane of u and vice versa -- one plane per field between
     those two ranks, kept in wrap buffers the generated kernel selects at the ends;
  4. the generated forward / cotangent kernel on the owned cells (global indices for masks, windows and
     constant arrays), then the generated gathers, which write the rank's ghost-extended gradient: ghost
     planes receive what this rank's cells contribute to the NEIGHBOUR's cells, wrap buffers what they
     contribute across the ends;
  5. ("wrap") those wrap contributions are added into the owned end planes of the first / last rank;
  6. P^T down the levels WITHOUT exchanges.  The transpose is linear, so every rank pushes its own partial
     gradient -- owned planes plus the inner ghost plane of contributions -- through the unmodified whole-
     array P^T kernel: with the outer ghost planes zero, the wall weights of that kernel multiply zeros, and
     its result on the coarse owned planes and inner ghost planes is exactly this rank's share;
  7. ("halo") ONE packed message per neighbour carries the inner ghost planes of the gradients of all
     levels and fields; the receiver adds them to its owned boundary planes (transpose of step 1).  Levels too
     coarse to leave every rank 2 planes are AGGLOMERATED: every rank holds the whole array, prolongates from
     its window of it, pushes its share of the gradient into a zeroed copy, and one ("sum") all-reduce of
     those few small arrays replaces their halo-add; all ranks then apply the same update;
  8. ("sum") parameter gradients of networks / Arrays, when there are any; Adam on the packed vector.
The loss needs one more ("sum") of a few scalars, issued only when a value is read.

The epoch is a generator that yields at exchanges (`(kind, send_lo, send_hi)`), so the same code runs one rank
per GPU over RCCL (slab.TorchDistComm), over gloo with CPU doubles of the kernels (tests/test_slab_traced_cpu.py)
and with all ranks emulated in one process on one GPU (slab.run_lockstep, tests/test_slab_gpu.py).
"""

import contextlib
import math

import numpy as np
import torch

from . import ops as hip_ops
from .stencil_bind import StencilBinding, field_ranges
from .stencil_jit import trace_outputs
from .stencil_trace import TraceUnsupported

G = 2  # ghost planes per interior interface (the generated gathers assume 2)


class _Level:
    """One level array of one grid field on one rank."""

    def __init__(self, gshape, axis, rank, world, replicate=False):
        self.gshape, self.axis = tuple(gshape), axis
        self.rank, self.world = rank, world
        # A level with fewer than 2 planes per rank is AGGLOMERATED: every rank keeps the whole (small) array, computes
        # it redundantly and the ranks' gradient contributions are summed by one all-reduce.
        self.replicated = replicate or gshape[axis] % world != 0 or gshape[axis] // world < 2
        if self.replicated:
            self.n, self.g_lo, self.g_hi, self.off = gshape[axis], 0, 0, 0
        else:
            self.n = gshape[axis] // world
            self.g_lo = 0 if rank == 0 else G
            self.g_hi = 0 if rank == world - 1 else G
            self.off = rank * self.n
        self.shape = tuple(self.g_lo + self.n + self.g_hi if d == axis else s for d, s in enumerate(gshape))
        self.size = math.prod(self.shape)
        self.plane = self.size // self.shape[axis]

    def window_of(self, fine):
        """(first plane, count) of THIS (replicated, coarse) level that prolongates to the ghost-extended planes
        of the sharded level `fine` of this rank: half its owned range plus one plane per interior interface."""
        e_lo, e_hi = (1 if fine.g_lo else 0), (1 if fine.g_hi else 0)
        return fine.off // 2 - e_lo, fine.n // 2 + e_lo + e_hi

    def planes(self, a, first, count=1):
        """`count` planes from owned-relative position `first` along the sharded axis."""
        return a.narrow(self.axis, self.g_lo + first, count)

    def owned(self, a):
        return a.narrow(self.axis, self.g_lo, self.n)

    def inner(self, a):
        """View with ONE ghost plane per interior interface: the coarse operand of P, the result of P^T."""
        lo = self.g_lo - 1 if self.g_lo else 0
        hi = a.shape[self.axis] - (self.g_hi - 1 if self.g_hi else 0)
        return a.narrow(self.axis, lo, hi - lo)

    def plane_desc(self, start, pos, count=1):
        """(base, outer, ostride, inner) of the `count` planes from owned-relative position `pos` inside the packed vector
        whose entry `start` is this array's first element: `outer` runs of `inner` contiguous elements (ops.PlaneList)."""
        outer = math.prod(self.shape[:self.axis])
        inner = self.plane // outer
        return (start + (self.g_lo + pos) * inner, outer, self.shape[self.axis] * inner, inner * count)


class _Entry:
    """One unknown of the state in the packed vectors.  kind "mg" / "field": grid arrays, one `_Level` each in `levels`
    (`loc`: the field's); kind "par": the arrays of a network / Array, whole on every rank (`levels` is empty).  `shapes`:
    of its arrays as this rank stores them, one after the other from entry `start`.  `factors`: the multigrid factors
    when one of them is not 1, else None.  `init`: the state's arrays (initial values; dropped once copied).  x, m, v, g, h:
    one view per array of the run's packed vectors, attached by `SlabTracedAdam`."""

    def __init__(self, key, kind, init, levels=(), loc=None, factors=None):
        self.key, self.kind, self.init, self.levels, self.loc, self.factors = key, kind, list(init), list(levels), loc, factors
        self.shapes = [lv.shape for lv in levels] if levels else [tuple(a.shape) for a in init]
        self.start = None
        self.x = self.m = self.v = self.g = self.h = ()

    @property
    def synthesised(self):
        """Whether what the kernels read is u = w_0 + P(w_1 + ...), an array of its own, and not the unknown itself."""
        return self.kind == "mg" and len(self.levels) > 1

    def arrays(self):
        """(first entry, size, shape, level or None) of each of its arrays."""
        pos = self.start
        for k, shape in enumerate(self.shapes):
            yield pos, math.prod(shape), shape, self.levels[k] if self.levels else None
            pos += math.prod(shape)


class SlabLayout:
    """Where one rank's unknowns live -- host arithmetic only: no device allocation, no kernels.

    entries, by_key   the `_Entry` of every field of the state, in `Domain.arrays_from_state` order
    total             length of a packed vector
    rep               [(start, size)] of the replicated (agglomerated) level arrays
    n_owned, n_unknowns_local   entries of the owned planes of the sharded arrays; those plus every entry the rank holds
                      whole (replicated levels, parameters)
    The plane descriptors (`_Level.plane_desc`; side "lo" / "hi", absent at an end of the decomposition), every list in the
    order of the sharded level arrays in the packed vector:
    x_send, x_recv    the unknowns' halo: the owned boundary plane of every array out, the inner ghost plane in
    g_send, g_add     the gradients' halo-add, [0] the finest level of every field, [1] the coarser levels: per array the
                      inner ghost plane THEN the owned boundary plane out; added to the owned boundary plane THEN the inner
                      ghost plane (the second of each pair is the redundant update's, see SlabTracedAdam)."""

    def __init__(self, domain, state, axis, rank, world):
        from .core import Field, MultigridField

        grid = {k: f for k, f in state.fields.items() if isinstance(f, (Field, MultigridField))}
        if axis is None:
            ok = [d for d in range(domain.ndim) if all(f.loc[d] == "c" for f in grid.values())]
            if not ok:
                raise ValueError("no axis on which every field is cell-centred")
            axis = ok[0]
        N = domain.cshape[axis]
        if N % world:
            raise ValueError("{} cells on axis {} over {} ranks".format(N, axis, world))
        self.axis, self.rank, self.world, self.n = axis, rank, world, N // world
        self.entries = [self._entry(domain, key, f) for key, f in state.fields.items()]
        self.by_key = {e.key: e for e in self.entries}
        self.total = 0
        for e in self.entries:
            e.start = self.total
            self.total += sum(math.prod(s) for s in e.shapes)
        arrays = [a for e in self.entries for a in e.arrays()]
        # (first entry, level, whether it is the field's finest) of every array cut into slabs
        self.sharded = [(pos, lv, k == 0) for e in self.entries for k, (pos, _, _, lv) in enumerate(e.arrays())
                        if lv is not None and not lv.replicated]
        self.rep = [(pos, cnt) for pos, cnt, _, lv in arrays if lv is not None and lv.replicated]
        self.n_owned = sum(lv.n * lv.plane for _, lv, _ in self.sharded)
        self.n_unknowns_local = self.n_owned + sum(cnt for _, cnt, _, lv in arrays if lv is None or lv.replicated)
        self.global_cells = math.prod(domain.cshape)
        self.local_cells = self.global_cells // world
        self.x_send, self.x_recv = dict(), dict()
        self.g_send, self.g_add = (dict(), dict()), (dict(), dict())
        for side in ["lo"] * (rank > 0) + ["hi"] * (rank < world - 1):
            # (finest?, owned boundary plane, inner ghost plane) of every sharded array at this side
            pairs = [(top, lv.plane_desc(pos, 0 if side == "lo" else lv.n - 1),
                      lv.plane_desc(pos, -1 if side == "lo" else lv.n)) for pos, lv, top in self.sharded]
            self.x_send[side] = [own for _, own, _ in pairs]
            self.x_recv[side] = [ghost for _, _, ghost in pairs]
            # the same planes split by level for the gradients' halo-add: the finest levels (97 % of the bytes) travel WHILE
            # the transposes run down the levels, the coarser ones after them.  The message carries what this rank's cells
            # contribute to the neighbour's boundary plane (the ghost plane) and, for the redundant ghost updates, this
            # rank's own boundary plane of the partial gradient, which completes the receiver's inner ghost plane
            for k in (0, 1):
                self.g_send[k][side] = [d for top, own, ghost in pairs if top == (k == 0) for d in (ghost, own)]
                self.g_add[k][side] = [d for top, own, ghost in pairs if top == (k == 0) for d in (own, ghost)]

    def _entry(self, domain, key, f):
        """The entry of field `key`, or the reason why the decomposition cannot hold it."""
        from .core import Array, Field, MultigridField, NeuralNet

        axis, rank, world = self.axis, self.rank, self.world
        N = domain.cshape[axis]
        if isinstance(f, MultigridField):
            factors = [float(x) for x in (f.factors or domain.mg_factors or [1] * len(f.terms))]
            mgloc = domain._mg_loc(f)
            if mgloc[axis] != "c":
                raise ValueError("field '{}' is not refined / cell-centred on the sharded axis".format(key))
            levels = [_Level(tuple(t.array.shape), axis, rank, world) for t in f.terms]
            for l in range(len(levels) - 2, -1, -1):  # a rank's planes must be whole coarse cells at the transition
                if levels[l + 1].replicated and not levels[l].replicated and levels[l].n % 2:
                    levels[l] = _Level(tuple(f.terms[l].array.shape), axis, rank, world, replicate=True)
            if levels[0].replicated or any(a.replicated and not b.replicated for a, b in zip(levels, levels[1:])):
                raise ValueError("field '{}': {} cells on the sharded axis over {} ranks".format(key, N, world))
            # u = f_0 w_0 + P(f_1 w_1 + P(...)) (reference core.py:245-263); None: every factor is 1
            if len(levels) == 1 and factors[0] != 1.0:
                raise NotImplementedError("slab decomposition of a one-level multigrid field with a factor")
            return _Entry(key, "mg", [t.array for t in f.terms], levels, mgloc,
                          None if all(x == 1.0 for x in factors) else factors)
        if isinstance(f, Field):
            if f.loc[axis] != "c":
                raise ValueError("field '{}' is not cell-centred on the sharded axis".format(key))
            levels = [_Level(tuple(f.array.shape), axis, rank, world)]
            if levels[0].replicated:
                raise ValueError("field '{}': {} cells on the sharded axis over {} ranks".format(key, N, world))
            return _Entry(key, "field", [f.array], levels, f.loc)
        if isinstance(f, (NeuralNet, Array)):
            return _Entry(key, "par", domain.arrays_from_field(f))
        raise TypeError(type(f).__name__)

    def local_index(self, device=None):
        """Indices into a packed vector of what `n_unknowns_local` counts: the owned planes of the sharded arrays (`n_owned`
        entries), then what every rank holds whole."""
        own, rep = [], [torch.zeros(0, dtype=torch.int64, device=device)]
        for e in self.entries:
            for pos, cnt, shape, lv in e.arrays():
                index = torch.arange(pos, pos + cnt, dtype=torch.int64, device=device).view(shape)
                if lv is not None and not lv.replicated:
                    own.append(lv.owned(index).reshape(-1))
                else:
                    rep.append(index.reshape(-1))
        return torch.cat(own + rep)


def fused_update_plan(layout, keys, reread=()):
    """The optimizer's update inside the gathers.  A gather completes the gradient of the owned planes 1 .. n - 2 of its
    array (plane 0 / n - 1 wait for the neighbour's share or the periodic closure): the kernels that can, update those
    entries where they form the gradient, and the launches at the end of the epoch cover the rest of the packed vector --
    the two end pieces of every such array (strided when the sharded axis is not the leading one) and the ranges between
    the arrays (coarser levels, fields without a gather, parameters).
    keys: the fields whose gathers can update in place; reread: those whose own arrays the gathers read again.
    -> (fused: key -> (first, last + 1) owned plane updated by the gather, post_flat: [(begin, end)] for `ops.adam_step`,
    post_pieces: [(start, size, npieces, stride, offset, count)] for `ops.adam_step_pieces` on [start, start + size))."""
    fused, post_flat, post_pieces, spans = dict(), [], [], []
    for e in (layout.by_key[key] for key in keys):
        lv = e.levels[0]
        if lv.n < 4:
            continue
        if not e.synthesised and e.key in reread:
            continue  # the array a gather reads IS the unknown: no launch of this epoch may update it
        if e.factors:
            continue  # the gather forms h_0, the gradient is f_0 h_0
        fused[e.key] = (1, lv.n - 1)
        spans.append((e.start, lv.size))
        _, outer, stride, inner = lv.plane_desc(0, 0)
        first, last = lv.g_lo + 1, lv.g_lo + lv.n - 1  # planes [0, first) and [last, extent) of the array
        post_pieces.append((e.start, lv.size, outer, stride, 0, first * inner))
        post_pieces.append((e.start, lv.size, outer, stride, last * inner, (lv.shape[lv.axis] - last) * inner))
    at = 0
    for start, size in sorted(spans):
        if start > at:
            post_flat.append((at, start))
        at = start + size
    if at < layout.total:
        post_flat.append((at, layout.total))
    return fused, post_flat, post_pieces


class HipSlabKernels(StencilBinding):
    """The generated kernels of one rank (stencil_codegen in slab mode) and their buffers: the binding of stencil_bind.py,
    plus the geometry of the rank's slab and the wrap planes across the ends of the decomposition.

    THE INTERFACE `SlabTracedAdam` drives (a stand-in handed in as `kernels=` declares all of it, see
    tests/slab_traced_double.py):
      halo                      planes the operator reads away along the sharded axis (0 or 1)
      src_keys, gather_keys     grid fields the kernels read / whose gradient a gather forms
      merged                    the gather keys that `gather_all` serves in one launch (empty: `gather` per key)
      reread                    fields whose own arrays the gathers read again
      fused_adam                whether `gather(..., adam=)` / `gather_all(..., hyper)` can apply the optimizer's update
      param_groups, pgrad       key -> (offset, lengths) of the parameter gradients in the flat partial sums `pgrad`
      par_outputs               outputs in parameter space, or None; with them `pout` and `launch_par`
      set_geometry, set_params, forward, gather, partial_terms
    and, for Newton only (jac=True), jac_items and jacobian.  Of `ops` the driver calls interp_add, interp_adj_best,
    adam_step, adam_step_pieces (only with `fused_adam`) and PlaneList."""

    def __init__(self, problem, state, axis, n, device, jac=False):
        """jac: also generate `k_jac` (`jacobian`), in a library of its own -- the library of the gradient optimizers keeps
        its source and cache key."""
        tr, outs, raw, self.names, Gshape = trace_outputs(problem, state)

        # outputs in parameter space (a weight regulariser): every rank evaluates them, redundantly, with the generated
        # kernel of param_expr.py AFTER the parameter gradients were summed over the ranks
        def refuse(e):
            raise TraceUnsupported("outputs in parameter space under the slab decomposition ({})".format(e))

        super().__init__(problem, state, tr, outs, raw, Gshape, (axis, n), jac, device, refuse)
        cg = self.cg
        self.halo = cg.halo
        # global array index -> (field key, position among the field's arrays)
        self.par_where = {i: (key, i - pos) for key, _, pos, cnt in field_ranges(problem.domain, state)
                          for i in range(pos, pos + cnt)}
        self.args.alo = self.args.ahi = 0
        self.src_keys, self.gather_keys = list(cg.src_keys), list(cg.gathers)
        # fields whose own arrays the gathers read again (local derivatives re-evaluated there, stencil_grad.py)
        self.reread = {k for keys in cg.gather_reads_sources.values() for k in keys}
        self.merged = list(cg.merged)
        self.param_groups = {key: (cg.pg_offset[key], [len(g) for g in groups]) for key, groups in cg.pgrads.items()}
        self.jac_items = list(cg.jac_items)
        if self.jac_items:
            self.jac_buf = torch.empty((len(self.jac_items),) + tuple(cg.GL), dtype=self.dtype, device=device)

    def set_geometry(self, off, lo, ea):
        self.args.off, self.args.lo, self.args.ea, self.args.hw = off, lo, ea, self.halo

    def set_params(self, state_arrays_of):
        """Pointers of network / Array parameters (`state_arrays_of(key)` -> this rank's replicated arrays)."""
        i = 0
        for key, _ in self.cg.nets:
            for arr in state_arrays_of(key):
                self.args.par[i] = arr.data_ptr()
                i += 1
        for key, _ in self.cg.arrays:
            self.args.par[i] = state_arrays_of(key)[0].data_ptr()
            i += 1

    def _bind(self, srcs, wlo, whi):
        """The argument block filled for one evaluation: host scalars, sources and their wrap planes (src key -> array)."""
        from ._lib import ptr

        ptr(self.out)  # fails loudly on a CPU tensor: there is no CPU path
        self.refresh_host_scalars()
        for i, key in enumerate(self.src_keys):
            self.args.src[i] = srcs[key].data_ptr()
            self.args.wlo[i], self.args.whi[i] = wlo[key].data_ptr(), whi[key].data_ptr()

    def forward(self, srcs, wlo, whi):
        """Forward + cotangents on the owned cells.  srcs / wlo / whi: src key -> array."""
        self._bind(srcs, wlo, whi)
        self.fwd()

    def jacobian(self, srcs, wlo, whi):
        """`k_jac` on the owned cells (one launch): the value of every output and d output / d read for every distinct
        read, in the order of `self.jac_items` ((output, None) for a value, (output, read attr) for a derivative), as the
        leading slices of ONE buffer of shape [len(jac_items), *owned shape] -- reused by the next call.  srcs / wlo /
        whi as in `forward`: u after the halo exchange, the wrap planes across the ends of the decomposition."""
        self._bind(srcs, wlo, whi)
        self.jac(self.jac_buf)
        return self.jac_buf

    fused_adam = True  # gather() can apply the optimizer's update to the planes whose gradient it completes

    def gather(self, key, g, gwlo, gwhi, adam=None):
        """Ghost-extended gradient of field `key` (level 0) into g, wrap contributions into gwlo / gwhi.
        adam = (x, m, v, alpha, one_minus_b1, one_minus_b2, eps, lo, hi): Adam (reference optimizer.py:316-318) of the
        array's entries on the owned planes lo <= plane < hi of the sharded axis, by the lane that forms their gradient
        (x, m, v laid out as g)."""
        i = self.src_keys.index(key)
        self.args.gwlo[i], self.args.gwhi[i] = gwlo.data_ptr(), gwhi.data_ptr()
        self.args.alo = self.args.ahi = 0
        if adam is not None:
            x, m, v = adam[:3]
            assert x.shape == g.shape and x.is_contiguous() and m.is_contiguous() and v.is_contiguous()
            self.args.alo, self.args.ahi = int(adam[7]), int(adam[8])
            adam = adam[:7]
        super().gather(self.gather_keys.index(key), g, adam)

    def gather_all(self, items, hyper=None, planes=(0, 0)):
        """Every merged field's ghost-extended gradient in ONE launch (see `gather`): items = [(key, g, gwlo, gwhi,
        (x, m, v) or None)] for exactly the keys of `self.merged`; hyper = (alpha, one_minus_b1, one_minus_b2, eps)."""
        by_key = {it[0]: it for it in items}
        lists = [], [], [], []  # g, x, m, v in the order of self.merged
        for key in self.merged:
            _, g, gwlo, gwhi, xmv = by_key[key]
            i = self.src_keys.index(key)
            self.args.gwlo[i], self.args.gwhi[i] = gwlo.data_ptr(), gwhi.data_ptr()
            if xmv is not None:
                x, m, v = xmv
                assert x.shape == g.shape and x.is_contiguous() and m.is_contiguous() and v.is_contiguous()
            for lst, t in zip(lists, (g,) + tuple(xmv or (None, None, None))):
                lst.append(t)
        self.args.alo, self.args.ahi = int(planes[0]), int(planes[1])
        super().gather_all(*lists, hyper=hyper)

    def partial_terms(self):
        """This rank's share of every loss term (sum over owned cells / GLOBAL count)."""
        return self.out[1:1 + self.nout]

    def launch_par(self, values_of, grads_of):
        """The parameter-space outputs: terms into self.pout, gradients added to (set in) the parameters' gradient views.
        values_of / grads_of: field key -> list of this rank's (replicated) arrays."""
        if self.par_outputs is None:
            return
        where = [self.par_where[index] for index in self.cg.par_index]
        self.par([values_of(key)[j] for key, j in where], [grads_of(key)[j] for key, j in where])


class _Section:
    """`with _Section(timers, name):` puts the launches inside between the event pair that `timers.section(name)` hands
    out (bench.py's Timers); timers None: nothing is recorded."""

    def __init__(self, timers, name):
        self.begin, self.end = timers.section(name) if timers is not None else (None, None)

    def __enter__(self):
        if self.begin is not None:
            self.begin.record()

    def __exit__(self, *exc):
        if self.end is not None:
            self.end.record()


class SlabTracedAdam:
    """One rank of the slab-decomposed Adam loop of a traced operator.

    problem: the GLOBAL problem (global Domain, operator, extra -- constant arrays in `extra` are global, they
    do not carry the sharded unknowns' time axis); state: the global state's STRUCTURE; its arrays give the
    initial values when they are real tensors and zeros when they live on the 'meta' device."""

    # REDUNDANT GHOST UPDATES: every rank applies the optimizer's update to its inner
    # ghost planes as well as to its own planes -- the gradient message carries, besides the sender's contribution to
    # the receiver's boundary plane, the sender's own boundary plane of the partial gradient, so both ranks hold
    # the same complete gradient of the shared planes (a + b on one side, b + a on the other: the same bits) and
    # make the same update with the same library kernel; the exchange of the updated unknowns at the start of every
    # epoch disappears (one initial synchronisation of the ghost planes remains, and one after `unknowns_changed`).
    # Same bytes, one exchange fewer.
    redundant = True

    def __init__(self, problem, state, rank, world, axis=None, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 device=None, kernels=None):
        domain = problem.domain
        self.problem, self.domain, self.rank, self.world = problem, domain, rank, world
        self.device = device if device is not None else domain.mod.device
        self.dtype = torch.float64 if np.dtype(domain.dtype) == np.float64 else torch.float32
        self.npdt = np.float64 if self.dtype == torch.float64 else np.float32
        lay = self.layout = SlabLayout(domain, state, axis, rank, world)
        self.axis, self.n, self.entries, self.by_key = lay.axis, lay.n, lay.entries, lay.by_key
        self.n_unknowns_local, self.local_cells, self.global_cells = lay.n_unknowns_local, lay.local_cells, lay.global_cells
        self._packed_vectors()
        self._exchange_lists()
        self.kern = (kernels or HipSlabKernels)(problem, state, lay.axis, lay.n, self.device)
        self.h = self.kern.halo
        if self.h > 1:
            raise TraceUnsupported("reads {} cells away along the sharded axis (the exchange keeps 1 plane)".format(self.h))
        self._source_buffers()
        self._wrap_lists()
        lv0 = self.by_key[self.kern.src_keys[0]].levels[0]
        self.kern.set_geometry(lv0.off, lv0.g_lo, lv0.shape[lay.axis])
        self.kern.set_params(lambda key: self.by_key[key].x)
        self.lr, self.b1, self.b2, self.eps = self.npdt(lr), self.npdt(beta_1), self.npdt(beta_2), epsilon
        self.t = 0
        self.has_params = any(e.kind == "par" for e in self.entries) and bool(self.kern.param_groups)
        self._fused, self._post_flat, self._post_pieces = fused_update_plan(
            lay, self.kern.gather_keys if self.kern.fused_adam else (), self.kern.reread)

    # ---- set-up ----------------------------------------------------------------------------------------
    def _packed_vectors(self):
        """x, m, v, g: all unknowns of the rank, the optimizer's moments and the gradient, each ONE vector with a view per
        array on the entries; the state's values copied into x."""
        mk = lambda: torch.zeros(self.layout.total, dtype=self.dtype, device=self.device)
        self.x, self.m, self.v, self.g = mk(), mk(), mk(), mk()
        # fields with multigrid factors: the UNSCALED cotangents h_l = (P^T)^l g_u travel down the levels, the gradient
        # of level l is g_l = f_l h_l -- a second packed vector with the layout of g
        self.hvec = mk() if any(e.factors for e in self.entries) else None
        self._x_synced = False  # whether the inner ghost planes of x hold the neighbours' boundary planes
        for e in self.entries:
            spans = [(slice(pos, pos + cnt), shape) for pos, cnt, shape, _ in e.arrays()]
            views = lambda buf: [buf[s].view(shape) for s, shape in spans]
            e.x, e.m, e.v, e.g = views(self.x), views(self.m), views(self.v), views(self.g)
            # where the gathers / transposes write: g itself, or the unscaled twin when the field has factors
            e.h = views(self.hvec) if e.factors else e.g
            for xk, src, lv in zip(e.x, e.init, e.levels or [None] * len(e.x)):
                if src is not None and src.device.type != "meta":
                    if lv is not None:
                        src = src.narrow(self.axis, lv.off - lv.g_lo, lv.shape[self.axis])
                    xk.copy_(src.to(device=self.device, dtype=self.dtype))
            e.init = None

    def _exchange_lists(self):
        """The layout's plane descriptors on the device: one launch packs / unpacks / adds every plane of every level and
        field of an exchange (odil_planes_copy); the send buffers of the exchange points are allocated once."""
        lay = self.layout
        lists = lambda descs: {s: hip_ops.PlaneList(d, self.device) for s, d in descs.items() if d}
        bufs = lambda pls: {s: torch.empty(pl.count, dtype=self.dtype, device=self.device) for s, pl in pls.items()}
        self._x_send, self._x_recv = lists(lay.x_send), lists(lay.x_recv)
        self._send_x = bufs(self._x_send)
        self._g_add, self._g_send = zip(*((lists(add), lists(send)) for add, send in zip(lay.g_add, lay.g_send)))
        self._send_g = [bufs(pls) for pls in self._g_send]

    def _source_buffers(self):
        """What the kernels read besides the unknowns.  The periodic closure's planes (`h` planes per field at each end):
        the four sets -- u received from across the low / high end, gradient contributions the gathers write for across
        them -- are each ONE buffer with a view per field, so a set travels as one message without a pack (or is filled
        by one copy).  The synthesised arrays u of the multigrid fields are views of ONE buffer too; the levels between
        the finest and the coarsest get work arrays."""
        mk = lambda shape: torch.zeros(shape, dtype=self.dtype, device=self.device)
        keys, hw = self.kern.src_keys, max(self.h, 1)
        lv0 = {key: self.by_key[key].levels[0] for key in keys}
        wshape = {key: tuple(hw if d == self.axis else s for d, s in enumerate(lv0[key].shape)) for key in keys}
        self._wsize = {key: math.prod(wshape[key]) for key in keys}
        self._wrapbuf = {name: mk(sum(self._wsize.values())) for name in ("lo", "hi", "glo", "ghi")}
        self.u, self.work, self.wrap, self._ustart = dict(), dict(), dict(), dict()
        woff = 0
        for key in keys:
            e = self.by_key[key]
            self.wrap[key] = {name: buf[woff:woff + self._wsize[key]].view(wshape[key]) for name, buf in self._wrapbuf.items()}
            woff += self._wsize[key]
            if e.synthesised:
                self.work[key] = [None] + [mk(lv.shape) for lv in e.levels[1:-1]] + [None]
            else:
                self.u[key] = e.x[0]
        synth = [key for key in keys if self.by_key[key].synthesised]
        self._uflat = mk(sum(lv0[key].size for key in synth))
        uoff = 0
        for key in synth:
            self.u[key] = self._uflat[uoff:uoff + lv0[key].size].view(lv0[key].shape)
            self._ustart[key] = uoff
            uoff += lv0[key].size

    def _wrap_lists(self):
        """The plane lists of the periodic closure (none when the operator reads no neighbour along the sharded axis)."""
        keys, h = self.kern.src_keys, self.h
        lv0 = {key: self.by_key[key].levels[0] for key in keys}
        end = lambda key, side: 0 if side == "lo" else lv0[key].n - h
        # the end planes of the synthesised arrays that close the periodic direction, as ONE message per side packed by
        # one launch (odil_planes_copy) -- when every source field is synthesised; else slices + torch.cat
        self._wrap_pack = None
        if h and all(self.by_key[key].synthesised for key in keys):
            self._wrap_pack = {side: hip_ops.PlaneList([lv0[key].plane_desc(self._ustart[key], end(key, side)) for key in keys],
                                                       self.device) for side in ("lo", "hi")}
        # where the wrap contributions of the gradients land: the first / last `h` owned planes of every gathered
        # field's finest level, in message order (odil_planes_copy, mode add): side -> [(list, packed vector)]
        self._wrap_add = dict(lo=[], hi=[])
        for side in ("lo", "hi") if h else ():
            off = 0
            for key in keys:
                e = self.by_key[key]
                if key in self.kern.gather_keys:
                    desc = lv0[key].plane_desc(e.start, end(key, side), h)
                    self._wrap_add[side].append((hip_ops.PlaneList([desc], self.device, start=off),
                                                 self.hvec if e.factors else self.g))
                off += self._wsize[key]

    # ---- pieces of the epoch -------------------------------------------------------------------------
    def unknowns_changed(self):
        """For whoever writes the owned planes of `x` from outside an epoch: the inner ghost planes are refreshed by the
        next evaluation."""
        self._x_synced = False

    @staticmethod
    def _pack(lists, vec, bufs):
        """The (lo, hi) messages of an exchange: the planes of `lists` out of the packed vector `vec` (None: no neighbour)."""
        return tuple(lists[s].pack(vec, bufs[s]) if s in lists else None for s in ("lo", "hi"))

    @staticmethod
    def _unpack(lists, vec, received, add):
        for side, recv in zip(("lo", "hi"), received):
            if recv is not None:
                (lists[side].unpack_add if add else lists[side].unpack)(vec, recv)

    def _field_streams(self, keys):
        """One side stream per field for the TRANSPOSE chains: the small, latency-bound
        launches at the coarse end of one field's chain overlap the long launches of another's -- config 5 as one rank:
        P^T chains 1.80 -> 1.69 ms; the prolongation chains gain nothing that way (2.68 -> 2.71) and stay on one stream.
        Returns [(key, stream or None)] and a function that joins the streams back into the current one."""
        if len(keys) < 2 or self.device.type != "cuda":
            return [(key, None) for key in keys], lambda: None
        cur = torch.cuda.current_stream()
        pool = self.__dict__.setdefault("_streams", [torch.cuda.Stream() for _ in range(4)])
        used = []
        for i, key in enumerate(keys):
            s_ = pool[i % len(pool)]
            if s_ not in [u for _, u in used]:
                s_.wait_stream(cur)
            used.append((key, s_))

        def join():
            for s_ in {u for _, u in used}:
                cur.wait_stream(s_)

        return used, join

    def _synthesise(self):
        for key in self.kern.src_keys:
            e = self.by_key[key]
            if not e.synthesised:
                continue
            L = len(e.levels)
            coarse = e.x[L - 1]
            fac = e.factors or [1.0] * L
            cscale = fac[L - 1]
            for l in range(L - 2, -1, -1):
                out = self.u[key] if l == 0 else self.work[key][l]
                fine, lvc = e.levels[l], e.levels[l + 1]
                if lvc.replicated and not fine.replicated:  # this rank's window of the replicated coarse field
                    operand = coarse.narrow(self.axis, *lvc.window_of(fine))
                else:
                    operand = lvc.inner(coarse)
                # (a view of the level array without its outer ghost planes: read in place by the marching kernels)
                hip_ops.interp_add(operand, e.loc, add=e.x[l], coarse_scale=cscale, add_scale=fac[l], out=out)
                coarse, cscale = out, 1.0

    def _end_planes(self, side):
        """The h owned planes of u at the low ('lo') / high end of each source field, as one message (for source fields
        that are no synthesised arrays, which `_wrap_pack` does not cover)."""
        parts = []
        for key in self.kern.src_keys:
            lv = self.by_key[key].levels[0]
            parts.append(lv.planes(self.u[key], 0 if side == "lo" else lv.n - self.h, self.h).reshape(-1))
        return torch.cat(parts)

    def _transpose_chain(self):
        plan, join = self._field_streams(list(self.kern.gather_keys))
        for key, s_ in plan:
            with (torch.cuda.stream(s_) if s_ is not None else contextlib.nullcontext()):
                self._transpose_field(key)
        join()

    def _transpose_field(self, key):
        e = self.by_key[key]
        fac = e.factors
        for l in range(1, len(e.levels)):
            lv, fine = e.levels[l], e.levels[l - 1]
            if lv.replicated and not fine.replicated:
                # this rank's share of the replicated level: zero but for the window its planes reach
                e.h[l].zero_()
                if fac:
                    e.g[l].zero_()
                view = lambda a: a.narrow(self.axis, *lv.window_of(fine))
            else:
                view = lv.inner
            dst = view(e.h[l])
            hip_ops.interp_adj_best(e.h[l - 1], e.loc, tuple(dst.shape), out=dst)  # (in place, also into a strided view)
            if fac:
                torch.mul(dst, fac[l], out=view(e.g[l]))

    def _sources_gen(self, refresh, timers=None):
        """What the generated kernels read, as a generator that yields at its exchanges: the inner ghost planes of the
        unknowns (refresh=True, or when they are not in step with the neighbours), the synthesised arrays u and the wrap
        planes across the ends."""
        if refresh or not self._x_synced:
            # the neighbours' boundary planes of the unknowns -> inner ghost planes: once, and whenever somebody else has
            # changed the unknowns -- the epochs update the ghost planes redundantly
            with _Section(timers, "halo"):
                received = yield ("halo",) + self._pack(self._x_send, self.x, self._send_x)
                self._unpack(self._x_recv, self.x, received, add=False)
                self._x_synced = True
        with _Section(timers, "mg_synth"):
            self._synthesise()
        if self.h:
            with _Section(timers, "halo"):
                yield from self._wrap_sources_gen()

    def _wrap_sources_gen(self):
        """The end planes of u across the periodic closure into the wrap buffers."""
        first, last = self.rank == 0, self.rank == self.world - 1
        if self._wrap_pack is not None and self.world == 1:
            # one rank: its high planes ARE what lies across the low end -- packed straight into place
            self._wrap_pack["hi"].pack(self._uflat, self._wrapbuf["lo"])
            self._wrap_pack["lo"].pack(self._uflat, self._wrapbuf["hi"])
            return
        if self._wrap_pack is not None:
            end = lambda side: self._wrap_pack[side].pack(self._uflat)
        else:
            end = self._end_planes
        recv_lo, recv_hi = yield ("wrap", end("lo") if first else None, end("hi") if last else None)
        if recv_lo is not None:
            self._wrapbuf["lo"].copy_(recv_lo.reshape(-1))
        if recv_hi is not None:
            self._wrapbuf["hi"].copy_(recv_hi.reshape(-1))

    def wrap_planes(self):
        """(wlo, whi): src key -> the wrap planes of u across the low / high end (filled by the last exchange)."""
        return {k: w["lo"] for k, w in self.wrap.items()}, {k: w["hi"] for k, w in self.wrap.items()}

    def evaluate_gen(self):
        """The loss terms of the current unknowns (forward kernel only, no gradient), as a generator that yields at its
        exchanges; afterwards the ghost planes, u and the wrap planes hold this state (what `HipSlabKernels.jacobian`
        reads)."""
        yield from self._sources_gen(True)
        self.kern.forward(self.u, *self.wrap_planes())

    def _hyper(self):
        """(alpha, 1 - beta_1, 1 - beta_2, epsilon) of the update this epoch makes (reference optimizer.py:311-319)."""
        t = self.npdt(self.t + 1)
        alpha = self.lr * np.sqrt(1 - self.b2**t) / (1 - self.b1**t)
        return (alpha, 1 - self.b1, 1 - self.b2, self.eps)

    def _gathers(self, fused, hyper):
        """The ghost-extended gradient of every gathered field's finest level (h_0) and its wrap contributions; the
        fields of `fused` updated on the planes whose gradient is complete.  hyper None: no update."""
        arrays = lambda key: (self.by_key[key].h[0], self.wrap[key]["glo"], self.wrap[key]["ghi"])
        xmv = lambda key: (self.by_key[key].x[0], self.by_key[key].m[0], self.by_key[key].v[0])
        merged = list(self.kern.merged)
        spans = {fused[key] for key in merged if key in fused}
        if merged and len(spans) <= 1:  # one launch for all of them (the fused planes are the same for every field)
            items = [(key,) + arrays(key) + (xmv(key) if key in fused else None,) for key in merged]
            self.kern.gather_all(items, hyper, spans.pop() if spans else (0, 0))
        else:
            merged = []
        for key in self.kern.gather_keys:
            if key in merged:
                continue
            if key in fused:
                self.kern.gather(key, *arrays(key), adam=xmv(key) + hyper + fused[key])
            else:
                self.kern.gather(key, *arrays(key))

    def _wrap_add_gen(self):
        """The gathers' contributions across the periodic closure, added where they belong."""
        first, last = self.rank == 0, self.rank == self.world - 1
        received = yield ("wrap", self._wrapbuf["glo"] if first else None, self._wrapbuf["ghi"] if last else None)
        # what arrives from across the low end belongs to this rank's FIRST owned planes, and vice versa
        for side, recv in zip(("lo", "hi"), received):
            if recv is not None:
                for plist, vec in self._wrap_add[side]:
                    plist.unpack_add(vec, recv.reshape(-1))

    def _scale_finest(self):
        """g_0 = f_0 h_0 (ghost planes included: this rank's share of the neighbour's)."""
        for key in self.kern.gather_keys:
            e = self.by_key[key]
            if e.factors:
                torch.mul(e.h[0], e.factors[0], out=e.g[0])

    def _sum_replicated_gen(self):
        """Agglomerated levels: the ranks' shares summed (every rank then updates alike)."""
        rep = self.layout.rep
        if rep and self.world > 1:
            total = yield ("sum", torch.cat([self.g[a:a + c] for a, c in rep]), None)
            off = 0
            for a, c in rep:
                self.g[a:a + c].copy_(total[off:off + c])
                off += c

    def _param_sums_gen(self):
        """The parameter gradients of networks / Arrays summed over the ranks, into the entries' gradient views."""
        if self.has_params:
            total = yield ("sum", self.kern.pgrad.clone(), None)
            for key, (ofs, lens) in self.kern.param_groups.items():
                for view, cnt in zip(self.by_key[key].g, lens):
                    view.copy_(total[ofs:ofs + cnt].view(view.shape))
                    ofs += cnt

    def _adam_tail(self, hyper):
        """Adam on what no gather has updated (`fused_update_plan`)."""
        for lo, hi in self._post_flat:
            hip_ops.adam_step(self.x[lo:hi], self.m[lo:hi], self.v[lo:hi], self.g[lo:hi], *hyper)
        for start, size, pieces, stride, offset, count in self._post_pieces:
            span = slice(start, start + size)
            hip_ops.adam_step_pieces(self.x[span], self.m[span], self.v[span], self.g[span], pieces, stride, offset,
                                     count, *hyper)

    # ---- one epoch -------------------------------------------------------------------------------------
    def epoch_gen(self, timers=None, update=True):
        """One Adam epoch as a generator that yields at its exchanges.  update=False: loss and gradient only (the
        quasi-Newton driver of slab_solvers.py) -- the ghost planes of the unknowns are refreshed first (somebody else
        changed the unknowns), no launch applies an update, and self.g is left complete on the owned planes, on the
        replicated levels and on the parameters."""
        yield from self._sources_gen(not update, timers)
        with _Section(timers, "forward"):
            self.kern.forward(self.u, *self.wrap_planes())
        hyper = self._hyper()
        with _Section(timers, "gather"):
            self._gathers(self._fused if update else dict(), hyper if update else None)
        if self.h and self.kern.gather_keys:
            with _Section(timers, "halo"):
                yield from self._wrap_add_gen()
        self._scale_finest()
        # the gradients' halo-add in two messages: the finest levels' ghost planes are final now -- they are POSTED and
        # travel while the transposes run down the levels (which read this rank's partial arrays only); the coarser
        # levels' planes follow after the chain
        with _Section(timers, "halo"):
            token = yield ("post",) + self._pack(self._g_send[0], self.g, self._send_g[0])
        with _Section(timers, "mg_synth_adj"):
            self._transpose_chain()
        with _Section(timers, "halo"):
            self._unpack(self._g_add[0], self.g, (yield ("wait", token, None)), add=True)
            received = yield ("halo",) + self._pack(self._g_send[1], self.g, self._send_g[1])
            self._unpack(self._g_add[1], self.g, received, add=True)
            yield from self._sum_replicated_gen()
        yield from self._param_sums_gen()
        if self.kern.par_outputs is not None:
            self.kern.launch_par(lambda key: self.by_key[key].x, lambda key: self.by_key[key].g)
        if update:
            self.t += 1
            with _Section(timers, "adam"):
                self._adam_tail(hyper)

    def epoch(self, comm, timers=None):
        gen = self.epoch_gen(timers)
        try:
            msg = next(gen)
            while True:
                msg = gen.send(comm.exchange(*msg))
        except StopIteration:
            pass

    def par_terms(self, combined=False):
        """[(position among the loss terms, value or None)] of the parameter-space outputs.  Every rank evaluates them
        alike, so they are counted ONCE: by rank 0 (emulated ranks sum their last_loss(), quasi-Newton ranks their local
        losses), or by every rank when its terms are `combined` over the ranks already; None: not counted here."""
        if self.kern.par_outputs is None:
            return []
        counted = self.rank == 0 or combined
        return [(k, self.kern.pout[2 * q] if counted else None) for q, (k, _) in enumerate(self.kern.par_outputs)]

    def last_terms(self, comm=None):
        """Global loss terms of the last evaluation (one small all-reduce)."""
        part = self.kern.partial_terms().clone()
        if comm is not None:
            part = comm.exchange("sum", part, None)
        terms = [float(v) for v in part]
        for k, value in self.par_terms(combined=comm is not None):
            terms.insert(k, 0.0 if value is None else float(value))
        return terms

    def last_loss(self, comm=None):
        return float(sum(self.last_terms(comm)))

    def owned_arrays(self):
        """This rank's part of every unknown array, in `Domain.arrays_from_state` order."""
        res = []
        for e in self.entries:
            res += [lv.owned(a) for lv, a in zip(e.levels, e.x)] if e.levels else list(e.x)
        return res


def optimize_slab(args, problem, state, callback=None, axis=None):
    """`odil.util.optimize(args, "adam", ...)` for a run started with one process per GPU (e.g. `python -m
    torch.distributed.run --nproc-per-node 8 examples/velocity_from_tracer/veltracer3d.py --slab 1`): every rank
    builds the same GLOBAL problem, owns a slab of it (this module) and runs `args.epochs` Adam epochs (or, with
    `--optimizer lbfgsb`, that many L-BFGS-B iterations: slab_solvers.SlabTracedLbfgs; with `--optimizer newton`, that many
    Newton steps of one cell-centred Field on a 3-D grid cut along axis 0: slab_solvers.SlabTracedNewton); the loss
    terms are all-reduced and logged by rank 0 every `args.report_every` epochs (the quantity the reference's
    callback reports, src/odil/util.py:337-467).  `callback(run, epoch, terms)` is called on every rank at those
    epochs.  Returns the rank's SlabTracedAdam (its `owned_arrays()` are the rank's part of the solution; dump
    them with `odil.write_raw_slab`)."""
    from .slab import init_distributed
    from .util import printlog

    rank, world, comm = init_distributed()
    kw = {name: getattr(args, "adam_" + name) for name in ("beta_1", "beta_2", "epsilon")
          if getattr(args, "adam_" + name, None) is not None}
    optname = getattr(args, "optimizer", "adam") or "adam"
    if optname == "newton":
        # refused on every rank alike, before anything is built or changed (slab_solvers.check_slab_newton)
        from .slab_solvers import check_slab_newton

        check_slab_newton(args, problem, state, axis=axis, world=world)
        kw["kernels"] = lambda *a: HipSlabKernels(*a, jac=True)
    run = SlabTracedAdam(problem, state, rank, world, axis=axis, lr=args.lr, **kw)
    every = getattr(args, "report_every", 0) or 0
    start = getattr(args, "epoch_start", 0)

    def report(epoch):
        terms = run.last_terms(comm)  # of the last evaluation
        if rank == 0:
            printlog("epoch={:05d} ranks={} loss={:.8g} terms={}".format(
                epoch, world, sum(terms), " ".join("{:.6g}".format(t) for t in terms)))
        if callback is not None:
            callback(run, epoch, terms)

    if optname == "newton":
        # Newton on the slabs (slab_solvers.SlabTracedNewton): an "epoch" is a step, its loss that of the state after it
        # (util.optimize_newton)
        from .slab_solvers import SlabTracedNewton

        newton = SlabTracedNewton(run, linsolver=getattr(args, "linsolver", "direct"),
                                  tol=getattr(args, "linsolver_tol", 1e-10), maxiter=getattr(args, "linsolver_maxiter", None))
        for epoch in range(start + 1, args.epochs + 1):
            status = newton.step(comm)
            if getattr(args, "linsolver_verbose", 0) and rank == 0:
                printlog(status)
            if every and (epoch % every == 0 or epoch == args.epochs):
                report(epoch)
        return run
    if optname == "lbfgsb":
        # L-BFGS-B on the slabs (slab_solvers.SlabTracedLbfgs): an "epoch" is an iteration, as in the undivided driver
        from .slab_solvers import SlabTracedLbfgs

        opts = {dst: getattr(args, src) for src, dst in (("bfgs_m", "m"), ("bfgs_pgtol", "pgtol"), ("bfgs_maxls", "maxls"))
                if getattr(args, src, None) is not None}
        count = [start]

        def each(_x):
            count[0] += 1
            if every and (count[0] % every == 0 or count[0] == args.epochs):
                report(count[0])

        SlabTracedLbfgs(run).minimize(comm, args.epochs - start, callback=each, **opts)
        return run
    if optname != "adam":
        raise NotImplementedError("optimizer '{}' on the slab decomposition (adam, lbfgsb)".format(optname))
    for epoch in range(start + 1, args.epochs + 1):
        run.epoch(comm)
        if every and (epoch % every == 0 or epoch == args.epochs):
            report(epoch)  # (the evaluation at the start of this epoch)
    return run


def shape_state(domain, state):
    """The structure `Domain.init_state` would give for `state`, with arrays on the 'meta' device (shapes only):
    what a rank needs of the GLOBAL state when the global arrays would not fit, or need not exist."""
    from .core import Array, Field, MultigridField, NeuralNet, State
    from .backend import torch_dtype

    dt = torch_dtype(domain.dtype)
    meta = lambda shape: torch.empty(tuple(shape), dtype=dt, device="meta")
    fields = dict()
    for key, f in state.fields.items():
        if f is None or isinstance(f, Field):
            loc = (f.loc if f is not None else None) or "c" * domain.ndim
            cshape = (f.cshape if f is not None else None) or domain.cshape
            if domain.multigrid and domain.mg_convert_all:
                terms = [Field(meta(domain._get_field_shape(cs, loc)), loc=loc, cshape=cs) for cs in domain.mg_cshapes]
                fields[key] = MultigridField(terms=terms, loc=loc, factors=domain.mg_factors, method=domain.mg_interp)
            else:
                fields[key] = Field(meta(domain._get_field_shape(cshape, loc)), loc=loc, cshape=cshape)
        elif isinstance(f, (NeuralNet, Array, MultigridField)):
            fields[key] = domain.init_field(f)
        else:
            raise TypeError(type(f).__name__)
    return State(fields=fields, initialized=True)
