"""Host side of ONE generated stencil library: from a traced operator to a loaded library with its buffers, its argument
block and its launches.  The single-GPU evaluator (stencil_jit.TracedOperator) and the kernels of one slab rank
(slab_traced.HipSlabKernels) are this binding plus what is their own: where the sources and gradients live.

The argument blocks (`struct Args`, `struct ParArgs`) are described once, by the generator (`_Codegen.args_layout`,
`par_args_layout`): the C text of the source and the ctypes structures here are both made from those lists.
"""

import ctypes
import time

import numpy as np
import torch

from . import ops, param_expr
from .stencil_codegen import _Codegen, _compile
from .stencil_trace import _HOST_BINARY, _HOST_UNARY

_P = ctypes.c_void_p
_PP = ctypes.POINTER(ctypes.c_void_p)
_ADAM = [_P] * 3 + [ctypes.c_double] * 4 + [_P]  # x, m, v, alpha, 1 - beta_1, 1 - beta_2, eps, alpha on the device
_ARGTYPES = dict(  # (launchers of stencil_codegen._launchers; all end with the stream)
    jit_fwd=[_P, _P], jit_gather=[ctypes.c_int, _P, _P, _P], jit_gather_adam=[ctypes.c_int, _P, _P] + _ADAM + [_P],
    jit_gather_all=[_P] + [_PP] * 4 + _ADAM[3:] + [_P], jit_jac=[_P, _PP, _P], jit_jac_batch=[_P, _P, ctypes.c_int, _P],
    jit_par=[_P, _P, _P], jit_par_batch=[_P, _P, ctypes.c_int, _P], jit_fwd_batch=[_P, ctypes.c_int, _P],
    jit_gather_batch=[ctypes.c_int, _P, _P, ctypes.c_int, _P])


def field_ranges(domain, state):
    """(key, field, first array, number of arrays) of every field, positions in `arrays_from_state` order."""
    pos = 0
    for key, field in state.fields.items():
        n = len(domain.arrays_from_field(field))
        yield key, field, pos, n
        pos += n


def ctypes_struct(name, members):
    """The ctypes mirror of the C struct that `stencil_codegen.struct_text(name, members)` defines."""
    return type(name, (ctypes.Structure,), dict(
        _fields_=[(m.name, m.ctype if m.length is None else m.ctype * m.length) for m in members]))


def _hyper(hyper):
    """(alpha, 1 - beta_1, 1 - beta_2, eps, alpha_dev) as the launchers take them: alpha a host number, or a device tensor
    (the step size of a replayed graph) passed by pointer."""
    alpha, omb1, omb2, eps = hyper
    adev = alpha.data_ptr() if isinstance(alpha, torch.Tensor) else None
    return (0.0 if adev else float(alpha), float(omb1), float(omb2), float(eps), adev)


class StencilBinding:
    """The generated kernels of one traced operator: source, library, buffers, argument block, launches."""

    def __init__(self, problem, state, tr, outs, raw, G, slab, jac, device, par_refused, batch=False):
        """tr, outs, raw, G: of `stencil_jit.trace_outputs`; slab, jac, batch: of `_Codegen`.  par_refused(e): called when
        the outputs in parameter space have no elementwise form (param_expr.Unsupported) -- it raises, or returns and leaves
        them to the caller (`par_outputs` stays None)."""
        from .core import Array, NeuralNet
        from .stencil_trace import TraceUnsupported

        if batch and batch != "params" and tr.offgrid:
            raise TraceUnsupported("batched forward kernel: outputs in parameter space")

        domain = problem.domain
        self.problem, self.domain, self.tr, self.raw, self.G = problem, domain, tr, raw, G
        # outputs in parameter space (param_tape.py): [(position, expression, slice of the tape it needs)]
        self.offgrid = [(k, e, tr.param_tape.slice_for(e.param_ids())) for k, e in tr.offgrid]
        self.param_tape = tr.param_tape
        cg = self.cg = _Codegen(tr, outs, raw, G, state, slab=slab, jac=jac, batch=batch)
        # ... as ONE generated kernel when the taped operations have an elementwise form (param_expr.py)
        self.par_outputs = None
        if self.offgrid:
            numel = {i: int(a.numel()) for i, a in enumerate(domain.arrays_from_state(state))}
            try:
                self.par_outputs = param_expr.convert(tr.param_tape, self.offgrid, numel)
            except param_expr.Unsupported as e:
                if batch:  # (the torch replay of a single run has no batched form)
                    raise TraceUnsupported("batched parameter kernel: parameter-space output evaluated by torch ({})".format(e))
                par_refused(e)
        if self.par_outputs is not None:
            cg.parameter_outputs(self.par_outputs, numel, {
                i: key for key, field, pos, n in field_ranges(domain, state) if isinstance(field, (NeuralNet, Array))
                for i in range(pos, pos + n)})
        self.source = cg.source()
        self.lib, self.lib_path = _compile(self.source, cg.flags)
        for name, argtypes in _ARGTYPES.items():
            if hasattr(self.lib, name):
                getattr(self.lib, name).argtypes = argtypes
        dt = self.dtype = tr.torch_dtype
        self.total, self.nout = cg.total, len(outs)
        self.nblocks = cg.fwd_blocks
        nout, npg = self.nout, len(cg.pg_decl)
        self.cot = [torch.empty(cg.GL, dtype=dt, device=device) for _ in range(cg.ncot)]
        self.part = torch.empty(max(1, nout * self.nblocks), dtype=dt, device=device)
        self.ppart = torch.empty(max(1, npg * self.nblocks), dtype=dt, device=device)
        self.part2 = torch.zeros(16 * (nout + npg), dtype=dt, device=device)
        self.out = torch.zeros(1 + 2 * nout, dtype=dt, device=device)
        self.pgrad = torch.zeros(max(1, npg), dtype=dt, device=device)
        # marching kernels: what their in-kernel sums of read cotangents hand across segments of rows / strips of columns
        self.edge = torch.zeros(max(1, cg.edge_numel), dtype=dt, device=device)
        a = self.args = ctypes_struct("Args", cg.args_layout())()
        for i, t in enumerate(tr.tensors):
            a.ten[i] = t.data_ptr()
        for i, t in enumerate(self.cot):
            a.cot[i] = t.data_ptr()
        for name in ("part", "ppart", "part2", "out", "pgrad", "edge"):
            setattr(a, name, getattr(self, name).data_ptr())
        a.nblocks, a.hs = self.nblocks, None
        if self.par_outputs is not None:
            self.par_args = ctypes_struct("ParArgs", cg.par_args_layout())()
            self.pout = torch.zeros(2 * len(self.par_outputs), dtype=dt, device=device)
            self.par_args.pout = self.pout.data_ptr()

    # ---- host scalars -----------------------------------------------------------------------
    def _host_value(self, n, memo):
        if n.idx in memo:
            return memo[n.idx]
        if n.op == "const":
            v = n.attr
        elif n.op == "tracer":
            v = self.problem.tracers[n.attr]
        elif n.op == "where":
            c, a, b = (self._host_value(x, memo) for x in n.args)
            v = a if c else b
        elif len(n.args) == 1:
            v = _HOST_UNARY[n.op](self._host_value(n.args[0], memo))
        else:
            v = _HOST_BINARY[n.op](self._host_value(n.args[0], memo), self._host_value(n.args[1], memo))
        memo[n.idx] = v
        return v

    def host_scalars(self):
        """Host scalars of the trace: functions of `problem.tracers`, evaluated in Python double as the
        operator itself would."""
        memo = dict()
        return [float(self._host_value(n, memo)) for n in self.cg.hs]

    def refresh_host_scalars(self):
        """Current host scalars -> the argument struct.  Every eager launch copies the struct, so epochs
        queued behind each other keep their own values however far the host runs ahead."""
        for i, v in enumerate(self.host_scalars()):
            self.args.hsv[i] = v

    # ---- launches (on the current stream; the argument block is copied by the launch) --------------------------------
    def _launch(self, name, *args):
        rc = getattr(self.lib, name)(*args, ops.stream_ptr())
        if rc != 0:
            raise RuntimeError("generated kernel launch failed ({}): hip error {}".format(name, rc))

    def fwd(self):
        """k_fwd, k_final, k_loss: cotangents, loss terms and norms, parameter gradients of the bound sources."""
        self._launch("jit_fwd", ctypes.byref(self.args))

    def gather(self, which, g, adam=None):
        """Gather number `which` (position in `cg.gathers`) into g.  adam = (x, m, v, alpha, one_minus_b1, one_minus_b2,
        eps): the Adam update (reference optimizer.py:316-318) by the lane that forms the gradient; alpha as in `_hyper`."""
        if adam is None:
            self._launch("jit_gather", which, ctypes.byref(self.args), g.data_ptr())
        else:
            self._launch("jit_gather_adam", which, ctypes.byref(self.args), g.data_ptr(), *(t.data_ptr() for t in adam[:3]),
                         *_hyper(adam[3:]))

    def gather_all(self, g, x=None, m=None, v=None, hyper=None):
        """Every field of `cg.merged` in one launch.  g: their gradient arrays in that order; x, m, v: the arrays the
        fused Adam update works on, None where a field gets none; hyper = (alpha, one_minus_b1, one_minus_b2, eps)."""
        nk = len(self.cg.merged)
        ptrs = [(_P * nk)(*[None if t is None else t.data_ptr() for t in (lst or [None] * nk)]) for lst in (g, x, m, v)]
        self._launch("jit_gather_all", ctypes.byref(self.args), *ptrs, *_hyper(hyper or (0.0, 0.0, 0.0, 0.0)))

    def jac(self, buf):
        """k_jac: the arrays of `cg.jac_items` into the leading slices of `buf` [len(jac_items), *cg.GL]."""
        n = len(self.cg.jac_items)
        if not n:
            raise RuntimeError("these kernels were generated without their Jacobian kernel (jac=False)")
        self._launch("jit_jac", ctypes.byref(self.args), (_P * n)(*[buf[j].data_ptr() for j in range(n)]))

    def par(self, vals, grads):
        """k_par behind k_loss: the parameter-space outputs -- terms and norms into `pout`, the loss, gradients added to
        (set in) `grads`.  vals, grads: the parameter arrays `cg.par_index` and their gradients."""
        for s_, (val, grad) in enumerate(zip(vals, grads)):
            if not val.is_contiguous() or val.dtype != self.dtype:
                raise RuntimeError("parameter arrays must be contiguous {} tensors".format(self.dtype))
            self.par_args.val[s_], self.par_args.grad[s_] = val.data_ptr(), grad.data_ptr()
        self._launch("jit_par", ctypes.byref(self.args), ctypes.byref(self.par_args))


class _StagingRing:
    """Blocks of host bytes on their way to launches that read them from DEVICE memory: a ring of `depth` slots, each a
    pinned block, a device block and an event recorded behind the launch that read it.  A slot is refilled only after its
    event has completed, so neither the pending copy nor a queued launch ever sees a block the host has since rewritten;
    with all slots in flight the host waits for the oldest."""

    def __init__(self, nbytes, device, depth):
        self.slots = [dict(host=torch.empty(nbytes, dtype=torch.uint8).pin_memory(),
                           dev=torch.empty(nbytes, dtype=torch.uint8, device=device), done=None) for _ in range(depth)]
        self.next = 0

    def take(self):
        """The next slot, free to be rewritten: fill slot["host"], then `upload(slot)`, launch, `release(slot)`."""
        slot = self.slots[self.next]
        self.next = (self.next + 1) % len(self.slots)
        if slot["done"] is not None:
            slot["done"].synchronize()  # (the launch that read this slot has run: its blocks may be rewritten)
        return slot

    @staticmethod
    def upload(slot):
        """Queues the copy of the slot's host block on the current stream; returns the device address."""
        slot["dev"].copy_(slot["host"], non_blocking=True)
        return slot["dev"].data_ptr()

    @staticmethod
    def release(slot):
        """Behind the last launch that reads the slot."""
        if slot["done"] is None:
            slot["done"] = torch.cuda.Event()
        slot["done"].record()


class JacobianBatch:
    """ONE launch of `k_jac_batch` for members of an ensemble whose operators generated the same source (so
    `jit_cache._compile` handed them the same library): every member keeps its own trace, argument block and host scalars,
    only the launch is shared.  The launch reads the members' argument blocks and output pointers from DEVICE memory: per
    call they are gathered from the members' ctypes structs into pinned host memory and copied on the current stream.

    Two linearisations may be queued back to back without a synchronise (the hazard `TracedOperator.graph_upload`
    describes for host scalars): the staging is a `_StagingRing` of `depth` slots."""

    depth = 4

    def __init__(self, members):
        """members: the `TracedOperator`s (generated with jac="batch") of one group, in the order of the launch."""
        first = members[0]
        if any(m.lib_path != first.lib_path for m in members):
            raise ValueError("JacobianBatch: members of one launch share one generated library")
        if not hasattr(first.lib, "jit_jac_batch"):
            raise RuntimeError("these kernels were generated without the batched Jacobian kernel (jac=\"batch\")")
        self.members, self.lib = list(members), first.lib
        self.nitems = len(first.cg.jac_items)
        self.asize = ctypes.sizeof(first.args)
        nb = len(members)
        self.abytes = nb * self.asize  # (a multiple of 8: the block holds pointers)
        nbytes = self.abytes + nb * self.nitems * ctypes.sizeof(_P)
        self.ring = _StagingRing(nbytes, first.out.device, self.depth)

    def pointer_table(self, outputs):
        """The members' output pointers as the launch wants them ([B, items] addresses), from outputs[b][j], the contiguous
        array item j of member b goes to: made once per set of buffers, `launch` copies the bytes."""
        table = np.empty((len(self.members), self.nitems), dtype=np.uint64)
        for b, (member, outs) in enumerate(zip(self.members, outputs)):
            assert len(outs) == self.nitems
            for j, t in enumerate(outs):
                if not t.is_contiguous() or t.dtype != member.dtype or tuple(t.shape) != tuple(member.G) or not t.is_cuda:
                    raise RuntimeError("JacobianBatch: outputs are contiguous {} arrays of shape {} on the device".format(
                        member.dtype, tuple(member.G)))
                table[b, j] = t.data_ptr()
        return table

    def launch(self, states, table):
        """k_jac_batch for `states` (one per member) into the arrays of `table` (`pointer_table`; the caller keeps them
        alive)."""
        slot = self.ring.take()
        base = slot["host"].data_ptr()
        keep = []
        for b, (member, state) in enumerate(zip(self.members, states)):
            keep.append(member.bind_fields(state))
            ctypes.memmove(base + b * self.asize, ctypes.addressof(member.args), self.asize)
        assert table.shape == (len(self.members), self.nitems) and table.dtype == np.uint64 and table.flags.c_contiguous
        ctypes.memmove(base + self.abytes, table.ctypes.data, table.nbytes)
        dev = self.ring.upload(slot)
        rc = self.lib.jit_jac_batch(dev, dev + self.abytes, len(self.members), ops.stream_ptr())
        if rc != 0:
            raise RuntimeError("generated kernel launch failed (jit_jac_batch): hip error {}".format(rc))
        self.ring.release(slot)
        del keep


class EpochBatch:
    """The forward and gather launches of one Adam epoch for members of an ensemble whose operators generated the same
    source (generated with batch=True: one library): ONE `jit_fwd_batch` (k_fwd, k_final, k_loss of all members) and ONE
    `jit_gather_batch` per gather (the merged gather where the generator made one).  As in `JacobianBatch` every member
    keeps its own trace and argument block and the launches read the blocks from DEVICE memory -- but here no pointer
    changes between epochs: member b's sources are its slices of packed arrays, its gradients go to its slices of the
    packed level-0 gradients, its `out` is row b of one packed [B, 1 + 2 nout] tensor.  So the blocks are staged ONCE, and
    again only when a member's bytes change: host scalars (`cg.hs`, functions of `problem.tracers`), which `launch`
    evaluates for the members that have any and compares with what the device holds.  Members without host scalars cost
    no host time per epoch, and their launches can be captured into a graph (`graphable`).  `Array` unknowns that the
    kernels read change nothing in that: member b's `args.par` points at its rows of packed parameter tensors, `args.ppart`
    and `args.pgrad` at its rows of packed partial sums and parameter gradients.  `NeuralNet` unknowns are such parameter
    arrays too (generated with batch="params"): per network its weights, then its biases, then the Arrays, the order of
    `a.par` in a single run.  Outputs in parameter space (`cg.par_outputs`): every member also has a `ParArgs` block -- val
    / grad: its slices of the packed parameters and of their gradients, pout: its row of a packed [B, 2 npar_out] tensor
    held here -- staged with the argument blocks, and `launch_par` runs `k_par_batch` of all members."""

    depth = 4

    def __init__(self, members, sources, grads, out, params=None, pgrad=None, par_vals=None, par_grads=None):
        """members: the `TracedOperator`s of one group, in the order of the launch.  sources[b]: the contiguous arrays
        member b reads, in the order of `cg.src_keys`; grads[b]: {field key: the contiguous array its gradient goes to};
        out: [B, 1 + 2 nout] contiguous, B the number of members here.  The caller keeps all of them alive.
        Members whose kernels read `Array` unknowns (`cg.arrays`): params[b]: {Array key: the contiguous array member b
        reads it from -- its row of a packed tensor}; pgrad[b]: the contiguous row of at least len(cg.pg_decl) elements its
        k_loss writes the parameter gradients to, in the order of `cg.pg_decl`.  The partial sums of those rows (`ppart`)
        are one packed [B, npg * nblocks] buffer held here.  For a network, params[b][key] is the list of its arrays
        (weights, then biases).  par_vals[b] / par_grads[b] (outputs in parameter space): the contiguous arrays of
        `cg.par_index`, in that order, and where their gradients go."""
        first = members[0]
        if any(m.lib_path != first.lib_path for m in members):
            raise ValueError("EpochBatch: members of one launch share one generated library")
        if not hasattr(first.lib, "jit_fwd_batch"):
            raise RuntimeError("these kernels were generated without the batched forward and gather kernels (batch=True)")
        cg, nb = first.cg, len(members)
        self.members, self.lib, self.nb = list(members), first.lib, nb
        assert tuple(out.shape) == (nb, 1 + 2 * first.nout) and out.is_contiguous() and out.dtype == first.dtype
        real = ctypes.c_double if first.dtype == torch.float64 else ctypes.c_float
        adam = type("AdamP", (ctypes.Structure,), dict(_fields_=[(n, _P) for n in "xmv"] + [
            (n, real) for n in ("alpha", "omb1", "omb2", "eps")] + [("alpha_dev", _P)]))
        gat = type("GatB", (ctypes.Structure,), dict(_fields_=[("g", _P * max(1, len(cg.gathers))), ("ad", adam)]))
        self.asize, self.gsize = ctypes.sizeof(first.args), ctypes.sizeof(gat)
        self.abytes = nb * self.asize  # (a multiple of 8: the block holds pointers)
        # which = -1: the merged gather; the fields it does not cover keep launches of their own
        self.which = ([-1] if cg.merged else []) + [gi for gi, key in enumerate(cg.gathers) if key not in cg.merged]
        self.ptrs = []
        npg = len(cg.pg_decl)
        reads_params = bool(cg.nets or cg.arrays)
        if reads_params and (params is None or pgrad is None):
            raise RuntimeError("EpochBatch: kernels that read parameter arrays need `params` and `pgrad`")
        self.ppart = torch.empty((nb, max(1, npg * cg.fwd_blocks)), dtype=first.dtype, device=out.device) if npg else None
        self.npar_out = len(first.par_outputs or ())
        self.pargs, self.pout, self.psize = [], None, 0
        if self.npar_out:
            if not hasattr(first.lib, "jit_par_batch"):
                raise RuntimeError("these kernels were generated without the batched parameter kernel (batch=\"params\")")
            if par_vals is None or par_grads is None:
                raise RuntimeError("EpochBatch: outputs in parameter space need `par_vals` and `par_grads`")
            self.pout = torch.zeros((nb, 2 * self.npar_out), dtype=first.dtype, device=out.device)
            self.psize = ctypes.sizeof(first.par_args)
        # the parameter arrays in the order of `a.par`: per network its weights then its biases, then the Arrays
        layout = [(key, [ni * no for ni, no in zip(layers[:-1], layers[1:])] + list(layers[1:])) for key, layers in cg.nets]
        layout += [(key, [numel]) for key, numel in cg.arrays]
        for b, member in enumerate(members):
            if member.nblocks != cg.fwd_blocks or len(sources[b]) != len(cg.src_keys):
                raise RuntimeError("EpochBatch: member {} does not match the generated launch".format(b))
            for t in list(sources[b]) + list(grads[b].values()):
                if not t.is_contiguous() or t.dtype != member.dtype or not t.is_cuda:
                    raise RuntimeError("EpochBatch: sources and gradients are contiguous {} arrays on the device".format(member.dtype))
            if reads_params:
                if (len(member.cg.pg_decl) != npg or [n for _, n in member.cg.arrays] != [n for _, n in cg.arrays]
                        or [tuple(l) for _, l in member.cg.nets] != [tuple(l) for _, l in cg.nets]):
                    raise RuntimeError("EpochBatch: member {} does not match the generated launch".format(b))
                row = pgrad[b]
                held = []
                for key, numels in layout:
                    given = params[b][key]
                    given = list(given) if isinstance(given, (list, tuple)) else [given]
                    if len(given) != len(numels):
                        raise RuntimeError("EpochBatch: member {}: '{}' has {} parameter arrays, the kernels read {}".format(
                            b, key, len(given), len(numels)))
                    held += list(zip(given, numels))
                for t, least in held + [(row, npg)]:
                    if not t.is_contiguous() or t.dtype != member.dtype or not t.is_cuda or t.numel() < least:
                        raise RuntimeError("EpochBatch: parameter arrays and their gradient rows are contiguous {} arrays on the "
                                           "device, no shorter than the kernels index them".format(member.dtype))
                assert len(held) == cg.par_arrays
                for i, (t, _) in enumerate(held):
                    member.args.par[i] = t.data_ptr()
                member.args.pgrad = row.data_ptr()
                if npg:
                    member.args.ppart = self.ppart[b].data_ptr()
                if member.part2.numel() < 16 * (member.nout + npg):  # (SEG partial sums per row of k_final)
                    raise RuntimeError("EpochBatch: member {}: `part2` is shorter than the rows of k_final".format(b))
            if self.npar_out:
                index = cg.par_index
                if member.cg.par_index != index or len(par_vals[b]) != len(index) or len(par_grads[b]) != len(index):
                    raise RuntimeError("EpochBatch: member {} does not match the generated parameter kernel".format(b))
                for s_, (i, val, grad) in enumerate(zip(index, par_vals[b], par_grads[b])):
                    for t in (val, grad):
                        if not t.is_contiguous() or t.dtype != member.dtype or not t.is_cuda or t.numel() < cg.par_numel[i]:
                            raise RuntimeError("EpochBatch: the arrays of the parameter kernel and their gradients are contiguous "
                                               "{} arrays on the device, no shorter than it indexes them".format(member.dtype))
                    member.par_args.val[s_], member.par_args.grad[s_] = val.data_ptr(), grad.data_ptr()
                member.par_args.pout = self.pout[b].data_ptr()
                self.pargs.append(member.par_args)
            for i, t in enumerate(sources[b]):
                member.args.src[i] = t.data_ptr()
            member.args.out, member.args.hs = out[b].data_ptr(), None
            for key, slot in cg.direct.items():  # (the cotangent of the field's only read IS its gradient)
                if key in grads[b]:
                    member.args.cot[slot] = grads[b][key].data_ptr()
            p = gat()  # (ad stays null: the slot of a level-0 update fused into the gather)
            for gi, key in enumerate(cg.gathers):
                p.g[gi] = grads[b][key].data_ptr()
            self.ptrs.append(p)
        self.hs_members = [b for b, member in enumerate(members) if member.cg.hs]
        self.graphable = not self.hs_members
        self.gbytes = nb * self.gsize  # (a multiple of 8 too; the ParArgs blocks follow)
        self.ring = _StagingRing(self.abytes + self.gbytes + nb * self.psize, out.device, self.depth)
        self.slot, self.dev, self.hs_values = None, None, dict()
        self.uploads, self.launches, self.host_seconds = 0, 0, 0.0  # blocks staged, calls of `launch`, host time in them

    def _stage(self):
        """All members' blocks -> a free slot of the ring -> the device (on the current stream)."""
        if self.slot is not None:
            self.ring.release(self.slot)  # (behind every launch that read the blocks staged before)
        slot = self.slot = self.ring.take()
        base = slot["host"].data_ptr()
        for b, (member, p) in enumerate(zip(self.members, self.ptrs)):
            ctypes.memmove(base + b * self.asize, ctypes.addressof(member.args), self.asize)
            ctypes.memmove(base + self.abytes + b * self.gsize, ctypes.addressof(p), self.gsize)
        for b, pa in enumerate(self.pargs):
            ctypes.memmove(base + self.abytes + self.gbytes + b * self.psize, ctypes.addressof(pa), self.psize)
        self.dev = self.ring.upload(slot)
        self.uploads += 1

    def launch(self):
        """k_fwd, k_final, k_loss and the gathers of all members on the current stream."""
        t0 = time.perf_counter()
        stale = self.dev is None
        for b in self.hs_members:  # (only these cost host time per epoch)
            values = self.members[b].host_scalars()
            if self.hs_values.get(b) != values:
                self.hs_values[b], stale = values, True
                for i, v in enumerate(values):
                    self.members[b].args.hsv[i] = v
        if stale:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("EpochBatch: the argument blocks are staged before a capture, not inside it")
            self._stage()
        stream = ops.stream_ptr()
        rc = self.lib.jit_fwd_batch(self.dev, self.nb, stream)
        if rc != 0:
            raise RuntimeError("generated kernel launch failed (jit_fwd_batch): hip error {}".format(rc))
        for which in self.which:
            rc = self.lib.jit_gather_batch(which, self.dev, self.dev + self.abytes, self.nb, stream)
            if rc != 0:
                raise RuntimeError("generated kernel launch failed (jit_gather_batch {}): hip error {}".format(which, rc))
        self.launches += 1
        self.host_seconds += time.perf_counter() - t0

    def launch_par(self):
        """k_par_batch of all members on the current stream, behind `launch` (which staged the blocks and the host scalars
        of this epoch) and behind whatever forms the gradients it adds to."""
        if not self.npar_out:
            return
        if self.dev is None:
            raise RuntimeError("EpochBatch: `launch_par` runs behind `launch`, which stages the argument blocks")
        t0 = time.perf_counter()
        rc = self.lib.jit_par_batch(self.dev, self.dev + self.abytes + self.gbytes, self.nb, ops.stream_ptr())
        if rc != 0:
            raise RuntimeError("generated kernel launch failed (jit_par_batch): hip error {}".format(rc))
        self.host_seconds += time.perf_counter() - t0
