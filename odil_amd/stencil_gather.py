"""The gathers of stencil_codegen.py: from the adjoints `k_fwd` stored to the gradient of every field (`k_gat_*`, one
launch per field or `k_gat_all` for all of them), with the optimizer's update by the lane that forms the gradient, and the
Jacobian coefficient arrays `k_jac`, which is a kernel of the same form, with `k_jac_batch`, its body for the members of an
ensemble in one launch; and, for Adam ensembles, the forward and gather kernels under heads of that kind (`k_fwd_batch`,
`k_final_batch`, `k_loss_batch`, `k_gat_*_batch`: `_epoch_batch_kernels`).  (The gathers of a marching kernel:
stencil_march.py.)
"""

import numpy as np

from . import stencil_grad
from .stencil_trace import TraceUnsupported


class _GatherKernels:
    """Methods of `stencil_codegen._Codegen`, emitted from `source()` after the forward kernel."""

    def _standard_gathers(self, S):
        if self.gathers_done:
            return
        self.gathers = []  # keys of the fields that need a gather launch
        self.gather_reads_sources = dict()  # key -> the gather reads the fields' own arrays (not only stored adjoints)
        self.direct = dict()  # key -> cot slot that already IS the gradient
        by_key = dict()  # key -> [(slot, read attr, coefficient expression or None)]
        for slot, n in enumerate(self.cots):
            by_key.setdefault(n.attr[0], []).append((slot, n.attr, None))
        for k, n in enumerate(self.cut_nodes):
            for ridx, coeff in self.cut_set[n.idx].items():
                attr = self.tr.nodes[ridx].attr
                by_key.setdefault(attr[0], []).append((len(self.cots) + k, attr, coeff))
        symbolic = dict()
        if self.all_regular:
            symbolic = self._gradient_terms()
        self.gather_blocks = dict()
        keys = list(by_key) + [k for k in symbolic if k not in by_key]
        for key in keys:
            reads = by_key.get(key, [])
            floc = self.state.fields[key].loc
            fshape = self._field_shape(key)
            only_legacy = all(adj is None or not any(self.tr.nodes[r].attr[0] == key for r in adj) for adj in self.out_adj)
            if (self.slab is None and only_legacy and len(reads) == 1 and reads[0][2] is None and not any(reads[0][1][1])
                    and reads[0][1][2] == floc):
                self.direct[key] = reads[0][0]
                continue
            gi = len(self.gathers)
            self.gathers.append(key)
            regular = tuple(fshape) == self.G and all(attr[2] == floc for _, attr, _ in reads)
            if key in symbolic and regular and symbolic[key] is not None:
                self._gather_symbolic(S, gi, key, symbolic[key])
                continue
            if self.slab is not None:
                self._gather_slab(S, gi, key, reads, floc, fshape)
                continue
            tot = int(np.prod(fshape))
            self.gather_blocks[gi] = (tot + 255) // 256
            S.append('extern "C" __global__ __launch_bounds__(NB) void k_gat_{}(const Args a, T* __restrict__ g, const AdamP ad) {{'.format(gi))
            S.append("  const int l = blockIdx.x * NB + threadIdx.x;")
            S.append("  if (l >= {}) return;".format(tot))
            rem = "l"
            for d in reversed(range(self.ndim)):
                if d == 0:
                    S.append("  const int j0 = {};".format(rem))
                else:
                    S.append("  const int j{} = {} % {};".format(d, rem, fshape[d]))
                    S.append("  const int q{} = {} / {};".format(d, rem, fshape[d]))
                    rem = "q{}".format(d)
            S.append("  T acc = (T)0;")
            for entry, (slot, attr, coeff) in enumerate(reads):
                _, shift, loc, _ = attr
                idx, valid = [], []
                for d in range(self.ndim):
                    ns, nr = fshape[d], self.G[d]
                    ext = max(ns, nr)
                    s_ = shift[d] % ext
                    if s_ > ext // 2:
                        s_ -= ext
                    pos = "j{}".format(d) if not (floc[d] == "c" and loc[d] == "n") else "(j{} + 1)".format(d)
                    e = pos if s_ == 0 else "wrap({} - ({}), {})".format(pos, s_, ext)
                    if floc[d] == "n" and loc[d] == "c":  # trimmed: the last padded position was dropped
                        name = "t{}_{}".format(entry, d)
                        S.append("  const int {} = {};".format(name, e))
                        valid.append("{} < {}".format(name, nr))
                        e = name
                    idx.append(e)
                load = "a.cot[{}][{}]".format(slot, self._offset(idx, self.G))
                if coeff is not None:  # a cut array: the stored adjoint times d(node) / d(read)
                    load = "({}) * {}".format(coeff, load)
                if valid:
                    load = "(({}) ? {} : (T)0)".format(" && ".join(valid), load)
                S.append("  acc = acc + {};".format(load))
            S.append("  g[l] = acc;")
            S.append("  adam_apply(ad, l, acc);")
            S.append("}")
        # every symbolic gather in ONE launch: the fields' expressions share most of what they read (stored seeds, each
        # other's arrays), a merged pass reads it once (tracer with three space dimensions: 52 -> 36 words per point)
        self.merged = []
        sym_keys = [key for key in self.gathers if key in symbolic and symbolic[key] is not None
                    and tuple(self._field_shape(key)) == self.G
                    and all(attr[2] == self.state.fields[key].loc for _, attr, _ in by_key.get(key, []))]
        if len(sym_keys) >= 2:
            self.merged = sym_keys
            nk = len(sym_keys)
            S.append("struct GatAll {{ T* g[{0}]; AdamP ad[{0}]; }};".format(nk))
            nblocks_all = self._gather_kernel(S, "k_gat_all", [(key, symbolic[key]) for key in sym_keys], "const GatAll ga",
                                              lambda k: "ga.g[{}]".format(k), lambda k: "ga.ad[{}]".format(k))
            S.append('extern "C" int jit_gather_all(const Args* a, void* const* g, void* const* x, void* const* m, void* const* v,')
            S.append('                               double alpha, double omb1, double omb2, double eps, const void* alpha_dev, void* stream) {')
            S.append("  GatAll ga;")
            S.append("  for (int k = 0; k < {}; ++k) {{".format(nk))
            S.append("    ga.g[k] = (T*)g[k];")
            S.append("    ga.ad[k] = AdamP{(T*)x[k], (T*)m[k], (T*)v[k], (T)alpha, (T)omb1, (T)omb2, (T)eps, (const T*)alpha_dev};")
            S.append("  }")
            self.gather_all_blocks = nblocks_all
            S.append("  hipLaunchKernelGGL(k_gat_all, dim3({}), dim3(NB), 0, (hipStream_t)stream, *a, ga);".format(nblocks_all))
            S.append("  return (int)hipGetLastError();")
            S.append("}")

    def _gather_symbolic(self, S, gi, key, root):
        """The gather of ONE regular field as a pointwise kernel over its gradient expression."""
        self.gather_blocks[gi] = self._gather_kernel(S, "k_gat_{}".format(gi), [(key, root)],
                                                     "T* __restrict__ g, const AdamP ad", lambda k: "g", lambda k: "ad")

    def _gather_kernel(self, S, name, items, params, G_, AD_, owned=False):
        """A pointwise kernel over the gradient expressions of `items` = [(field key, expression)] (one thread per
        point, or per four points of the last axis): common sub-expressions and loads of the fields' expressions are
        shared, every field's gradient is stored, and the optimizer's update applied, by the lane that holds it.
        Slab mode: threads cover planes -2 .. n + 2 of the sharded axis; planes that exist in the rank's ghost-extended
        gradient array are stored there (ghost planes: what this rank's cells contribute to the neighbour's), planes
        beyond an end of the decomposition that a periodic read reached go to the wrap buffers (as the legacy slab
        gather).  owned=True (slab mode, `k_jac`): threads cover the OWNED planes 0 .. n only, reads go through the same
        ghost / wrap addressing, and every item is stored into an array of the owned shape; no optimizer update.
        Returns the number of workgroups to launch."""
        vw, last = self.vw_gat, self.ndim - 1
        seen = dict()
        for _, root in items:
            for n in stencil_grad.subdag(root):
                seen[n.idx] = n
        nodes = [seen[i] for i in sorted(seen)]
        with self._body(order=nodes, vw=vw, in_gather=True) as gathered:
            self.forward()
            body = gathered.lines
            interior = self._interior_copy(nodes, vw)
            pre = gathered.pre + self._group_arrays()
        values = [self.r(root) for _, root in items]
        sources = sorted({n.attr[0] for n in nodes if n.op == "read" and not n.attr[0].startswith("@")})
        for key, _ in items:
            if not key.startswith("@"):  # (bookkeeping of the optimizer fusion: the items of the Jacobian kernel are no fields)
                self.gather_reads_sources[key] = sorted(set(self.gather_reads_sources.get(key, [])) | set(sources))
        shape = list(self.G)
        names = ["i{}".format(d) for d in range(self.ndim)]
        if self.slab is not None:
            ax, nloc = self.slab
            shape[ax] = nloc if owned else nloc + 4
            names[ax] = "jx"
        threads = int(np.prod(shape)) // vw
        if threads >= 2**31 - 1024:
            raise TraceUnsupported("grid too large for 32-bit indexing")
        flat = "l4" if vw == 4 else "l"
        S.append('extern "C" __global__ __launch_bounds__(NB) void {}(const Args a, {}) {{'.format(name, params))
        S.append(self._block_index(shape, vw))
        S.append("  const int {}r = bx_ * NB + threadIdx.x;".format(flat))
        S.append("  if ({}r >= {}) return;".format(flat, threads))
        self._chunk_remap(S, shape, vw, flat + "r", flat)
        self._index_prologue(S, shape, names, vw, flat)
        nblocks = (threads + 255) // 256
        if self.slab is not None and owned:
            S.append("  const int jo = jx;")
            S.append("  const int i{}g = jo + a.off;".format(ax))
        elif self.slab is not None:
            S.append("  const int jo = jx - 2;")  # owned-relative position on the sharded axis
            S.append("  const int i{}g = wrap(jo + a.off, {});".format(ax, self.G[ax]))
        S.extend(pre)
        for k in range(len(items)):
            S.append("  T acc{}[{}];".format(k, vw))

        def point_block(body_):
            B = []
            self._loop_open(B, vw)
            B.extend(body_)
            for k, value in enumerate(values):
                B.append("  acc{}[{}] = {};".format(k, "p" if vw == 4 else "0", value))
            if vw == 4:
                B.append("  }")
            return B

        if interior is None:
            S.extend(point_block(body))
        else:
            S.append("  if (__all((int)({}))) {{".format(self._interior_cond(interior[1][1])))
            S.extend(point_block(interior[0][0]))
            S.append("  } else {")
            S.extend(point_block(body))
            S.append("  }")
        adam = "adam_apply4({ad}, {o}, acc{k});" if vw == 4 else "adam_apply({ad}, {o}, acc{k}[0]);"
        put = "*(T4*)({dst} + {o}) = (T4){{acc{k}[0], acc{k}[1], acc{k}[2], acc{k}[3]}};" if vw == 4 else "{dst}[{o}] = acc{k}[0];"
        if vw == 4 and self.nt_streams:  # (with the optimizer state, see adam_apply4)
            put = "__builtin_nontemporal_store((T4){{acc{k}[0], acc{k}[1], acc{k}[2], acc{k}[3]}}, (T4*)({dst} + {o}));"
        if self.slab is None:
            o = "l4 * 4" if vw == 4 else "l"
            for k in range(len(items)):
                S.append("  " + put.format(dst=G_(k), o=o, k=k))
                S.append("  " + adam.format(ad=AD_(k), o=o, k=k))
            S.append("}")
            return nblocks

        def offset(along, extent):
            full = [along if d == ax else ("ib" if (vw == 4 and d == last) else "i{}".format(d)) for d in range(self.ndim)]
            ext = [extent if d == ax else self.G[d] for d in range(self.ndim)]
            return self._offset(full, ext)

        if owned:
            S.append("  const int o = {};".format(offset("jo", nloc)))
            for k in range(len(items)):
                S.append("  " + put.format(dst=G_(k), o="o", k=k))
            S.append("}")
            return nblocks
        S.append("  const int jl = jo + a.lo;")
        # owned planes a.alo <= jo < a.ahi have their whole gradient here (no neighbour's cell reads them): the optimizer's
        # update is applied on the spot; the planes next to an interface wait for the halo sum (slab_traced.py)
        S.append("  if (jl >= 0 && jl < a.ea) {")
        S.append("    const int o = {};".format(offset("jl", "a.ea")))
        for k in range(len(items)):
            S.append("    " + put.format(dst=G_(k), o="o", k=k))
            S.append("    if (jo >= a.alo && jo < a.ahi) " + adam.format(ad=AD_(k), o="o", k=k))
        S.append("  }")
        S.append("  else if (jo < 0 && jo >= -a.hw) {")
        S.append("    const int o = {};".format(offset("(jo + a.hw)", "a.hw")))
        for k, (key, _) in enumerate(items):
            S.append("    " + put.format(dst="a.gwlo[{}]".format(self.src_keys.index(key)), o="o", k=k))
        S.append("  }")
        S.append("  else if (jo >= {0} && jo < {0} + a.hw) {{".format(nloc))
        S.append("    const int o = {};".format(offset("(jo - {})".format(nloc), "a.hw")))
        for k, (key, _) in enumerate(items):
            S.append("    " + put.format(dst="a.gwhi[{}]".format(self.src_keys.index(key)), o="o", k=k))
        S.append("  }")
        S.append("}")
        return nblocks

    def _gather_slab(self, S, gi, key, reads, floc, fshape):
        """Gather of one field on one rank's slab.  Threads cover planes -2 .. n + 2 of the sharded axis (owned
        cells 0 .. n): g = sum_r cot_r[j - shift_r] over the OWNED cells that read j.  Planes that exist in the
        rank's ghost-extended gradient array are stored there (ghost planes: the part of the neighbour's gradient
        that this rank's cells produce, sent over and added by slab_traced.py); planes beyond a side WITHOUT ghosts
        (the ends of the decomposition) that a periodic read reached go to the wrap buffers gwlo / gwhi."""
        ax, nloc = self.slab
        slot = self.src_keys.index(key)
        per = [fshape[d] for d in range(self.ndim)]
        S.append('extern "C" __global__ __launch_bounds__(NB) void k_gat_{}(const Args a, T* __restrict__ g, const AdamP ad) {{'.format(gi))
        tot_per = int(np.prod([fshape[d] for d in range(self.ndim) if d != ax]))
        # 32-bit index arithmetic whenever the thread space fits (divisions by constants: a 64-bit one costs ~4x)
        it = "int" if tot_per * (nloc + 4) < 2**31 - 512 else "long"
        S.append("  const {0} l = ({0})blockIdx.x * NB + threadIdx.x;".format(it))
        S.append("  if (l >= ({}){} * {}) return;".format(it, tot_per, nloc + 4))
        rem = "l"
        for d in reversed(range(self.ndim)):
            ext = (nloc + 4) if d == ax else per[d]
            if d == 0:
                S.append("  const int j0 = (int){};".format(rem))
            else:
                S.append("  const int j{} = (int)({} % {});".format(d, rem, ext))
                S.append("  const {} q{} = {} / {};".format(it, d, rem, ext))
                rem = "q{}".format(d)
        S.append("  const int jo = j{} - 2;".format(ax))  # owned-relative position on the sharded axis
        S.append("  T acc = (T)0;")
        loads = []
        for entry, (cslot, attr, coeff) in enumerate(reads):
            _, shift, loc, _ = attr
            idx, valid = [], []
            for d in range(self.ndim):
                ns, nr = fshape[d], self.G[d]
                ext = max(ns, nr)
                s_ = shift[d] % ext
                if s_ > ext // 2:
                    s_ -= ext
                if d == ax:
                    # the load is UNCONDITIONAL on a clamped position and masked afterwards: loads behind per-entry
                    # branches are issued one at a time (each waits for the previous one's branch)
                    name = "c{}".format(entry)
                    S.append("  const int {} = jo - ({});".format(name, s_))
                    valid.append("{0} >= 0 && {0} < {1}".format(name, nloc))
                    idx.append("min(max({}, 0), {})".format(name, nloc - 1))
                    continue
                pos = "j{}".format(d) if not (floc[d] == "c" and loc[d] == "n") else "(j{} + 1)".format(d)
                e = pos if s_ == 0 else "wrap({} - ({}), {})".format(pos, s_, ext)
                if floc[d] == "n" and loc[d] == "c":
                    name = "t{}_{}".format(entry, d)
                    S.append("  const int {} = {};".format(name, e))
                    valid.append("{} < {}".format(name, nr))
                    e = "min({}, {})".format(name, nr - 1)  # (the masked load stays inside the array)
                idx.append(e)
            S.append("  const T w{} = a.cot[{}][{}];".format(entry, cslot, self._offset(idx, self.GL)))
            loads.append((entry, coeff, " && ".join(valid)))
        for entry, coeff, valid in loads:  # every load above is in flight before the first use
            term = "w{}".format(entry) if coeff is None else "({}) * w{}".format(coeff, entry)
            S.append("  acc = acc + (({}) ? {} : (T)0);".format(valid, term))

        def offset(along, extent):
            full = [along if d == ax else "j{}".format(d) for d in range(self.ndim)]
            shape = [extent if d == ax else per[d] for d in range(self.ndim)]
            return self._offset(full, shape)

        S.append("  const int jl = jo + a.lo;")
        # owned planes a.alo <= jo < a.ahi have their whole gradient here (no neighbour's cell reads them): the optimizer's
        # update is applied on the spot; the planes next to an interface wait for the halo sum (slab_traced.py)
        S.append("  if (jl >= 0 && jl < a.ea) {")
        S.append("    const int o = {};".format(offset("jl", "a.ea")))
        S.append("    g[o] = acc;")
        S.append("    if (jo >= a.alo && jo < a.ahi) adam_apply(ad, o, acc);")
        S.append("  }")
        S.append("  else if (jo < 0 && jo >= -a.hw) a.gwlo[{}][{}] = acc;".format(slot, offset("(jo + a.hw)", "a.hw")))
        S.append("  else if (jo >= {0} && jo < {0} + a.hw) a.gwhi[{1}][{2}] = acc;".format(nloc, slot, offset("(jo - {})".format(nloc), "a.hw")))
        S.append("}")

    def _jacobian_kernel(self, S):
        """`k_jac`: what `Problem.eval_operator_grad` returns (reference core.py:1313-1361, the input of `linearize`,
        core.py:1113-1217) as ONE pointwise kernel -- the value of every output and d output / d read for every distinct
        read (key, shift, loc), i.e. the per-shift coefficient arrays of the Jacobian -- from the SYMBOLIC derivative of the
        traced DAG (stencil_grad.GradBuilder with the unit seed), instead of one autograd pass per output over a graph
        of torch elementwise kernels.  Operators whose outputs are windows of the grid, or that differentiate through
        parameter arrays (dense Jacobian columns), keep the autograd route (TraceUnsupported).  Slab mode: the rank's owned
        cells only, u read from the ghost-extended array and the wrap planes, one owned-shape array per item
        (slab_traced.HipSlabKernels.jacobian)."""
        tr = self.tr
        items, self.jac_items = [], []  # jac_items[j] = (output position, None for its value | the read's attr)
        for k, o in enumerate(self.outputs):
            if o.win is not None or tuple(o.shape) != self.G or self.raw[k]:
                raise TraceUnsupported("Jacobian kernel: output {} is not a plain residual on the whole grid".format(k))
            nodes = stencil_grad.subdag(o)
            if not stencil_grad.differentiable(nodes, self.need):
                raise TraceUnsupported("Jacobian kernel: parameters below output {} (dense columns)".format(k))
            gb = stencil_grad.GradBuilder(tr, self.G, self.need, stop=())
            items.append(("@jv{}".format(k), gb.real(o)))
            self.jac_items.append((k, None))
            adj = gb.adjoints(o, gb.const(1.0), nodes) if self.need.get(o.idx, False) else dict()
            for ridx in sorted(adj):
                expr = adj[ridx]
                if expr is None:
                    continue
                items.append(("@jd{}_{}".format(k, ridx), expr))
                self.jac_items.append((k, tuple(tr.nodes[ridx].attr)))
        if len(items) > 96:
            raise TraceUnsupported("Jacobian kernel: {} arrays".format(len(items)))
        self.jac_exprs = [expr for _, expr in items]  # (what the kernel evaluates for jac_items[j]: tests/test_jacobian_kernel_host.py)
        S.append("struct JacP {{ T* p[{}]; }};".format(len(items)))
        first = len(S)
        self.jac_blocks = self._gather_kernel(S, "k_jac", items, "const JacP jp, const AdamP ad", lambda k: "jp.p[{}]".format(k),
                                              lambda k: "ad", owned=self.slab is not None)
        if self.jac_batch:
            self._jacobian_batch_kernel(S, S[first + 1:])

    def _jacobian_batch_kernel(self, S, body):
        """`k_jac_batch`: the body of `k_jac` (its lines as emitted, after the signature) for the B members of an ensemble
        whose operators gave this same source, on a grid (jac_blocks, B): workgroup (x, b) is workgroup x of member b's
        `k_jac`.  Every member has its own argument block and output pointers, in DEVICE memory (`ab[b]`, `jb[b]`:
        stencil_bind.JacobianBatch).  blockIdx.y is uniform over the workgroup and the blocks are not written while the
        kernel runs: they are read through the constant address space, i.e. by scalar loads of the members the body uses
        (no per-lane copy of the struct, no scratch), as `k_jac` reads its kernel arguments.  The XCD regrouping of
        `_block_index` reads gridDim.x / blockIdx.x only: every member keeps the schedule of its single launch."""
        S.append("typedef const __attribute__((address_space(4))) Args ArgsC;")
        S.append("typedef const __attribute__((address_space(4))) JacP JacPC;")
        S.append('extern "C" __global__ __launch_bounds__(NB) void k_jac_batch(const Args* __restrict__ ab, '
                 'const JacP* __restrict__ jb) {')
        S.append("  ArgsC& a = *(ArgsC*)(ab + blockIdx.y);")
        S.append("  JacPC& jp = *(JacPC*)(jb + blockIdx.y);")
        S.append("  const AdamP ad = {nullptr, nullptr, nullptr, (T)0, (T)0, (T)0, (T)0, nullptr};")
        S.extend(body)

    # ---- the forward and gather kernels for the members of an ensemble (batch=True) ---------------------------------
    def _epoch_batch_refusal(self, march):
        """TraceUnsupported for every kernel form that is not a pointwise body reading `a` alone (called from `source()`
        once the forward body is known)."""
        if march is not None:
            raise TraceUnsupported("batched forward kernel: the marching forward kernel hands sums across workgroups "
                                   "(`edge`), it is no pointwise body")
        # (`Array` unknowns pass: member b's `a.par`, `a.ppart` and `a.pgrad` are its own, and the rows of `pg_decl` are
        # reduced by the bodies of k_final / k_loss like the outputs' -- stencil_bind.EpochBatch; a network's parameter
        # arrays and their hundreds of rows have no packed home there)
        # batch="params": they have one -- a network's arrays are slices of the member's row of the packed parameters like
        # the Arrays (`W` / `Bv` read `a.par` of the member's block: no marching kernel here, so `wregs` is "mem"), and the
        # outputs in parameter space run as `k_par_batch`
        if self.batch_params:
            return
        if self.nets:
            raise TraceUnsupported("batched forward kernel: network or Array parameters (parameter gradients reduced over "
                                   "the grid)")
        if self.par_outputs:
            raise TraceUnsupported("batched forward kernel: outputs in parameter space")

    @staticmethod
    def _kernel_bodies(lines):
        """{name: (signature line, the lines after it up to and with the closing brace)} of the kernels in `lines`."""
        found, k = dict(), 0
        while k < len(lines):
            if lines[k].startswith('extern "C" __global__'):
                end = lines.index("}", k)
                name = lines[k].split(" void ", 1)[1].split("(", 1)[0]
                found[name] = (lines[k], lines[k + 1:end + 1])
                k = end
            k += 1
        return found

    def _epoch_batch_kernels(self, S, fwd_body, final_lines, gather_lines):
        """`k_fwd_batch`, `k_final_batch`, `k_loss_batch`, `k_gat_<i>_batch` and `k_gat_all_batch`: the bodies of the single
        kernels (their lines as emitted, after the signature) for the B members of an ensemble whose operators gave this
        same source, on a grid with one more dimension for the member -- the technique of `_jacobian_batch_kernel`: every
        member has its own argument block in DEVICE memory (`ab[member]`: its own sources, cotangent arrays, partial sums
        and `out`), read through the constant address space (scalar loads) -- here into a by-value `Args a`, so that the
        body is compiled on the values of a struct as the single kernel's is on its kernel argument: float kernels are
        built with -ffp-contract=fast, where WHICH products are fused depends on the code around them, and with `a` a
        reference into constant memory the forward kernel of a 12 x 18 float member fused two more (its loss differed
        from the single launch's in the last bit).  The member is the first grid dimension the body does not
        read: blockIdx.y (k_fwd, the gathers), blockIdx.z (k_final), blockIdx.x (k_loss); the XCD regrouping of
        `_block_index` reads gridDim.x / blockIdx.x only, so every member keeps the schedule, the partial sums and their
        order of its single launch.  The gathers take a `GatB` per member: the gradient array of every gather and ONE
        AdamP (null here: the slot of a fused level-0 update)."""
        finals, gathers = self._kernel_bodies(final_lines), self._kernel_bodies(gather_lines)
        ng = max(1, len(self.gathers))
        S.append("typedef const __attribute__((address_space(4))) Args ArgsC;")
        S.append("struct GatB {{ T* g[{}]; AdamP ad; }};".format(ng))
        S.append("typedef const __attribute__((address_space(4))) GatB GatBC;")

        def head(name, bounds, member, gat=False):
            S.append('extern "C" __global__ __launch_bounds__({}) void {}_batch(const Args* __restrict__ ab{}) {{'.format(
                bounds, name, ", const GatB* __restrict__ gb" if gat else ""))
            S.append("  Args a;")
            S.append("  __builtin_memcpy(&a, (ArgsC*)(ab + {}), sizeof(Args));".format(member))
            if gat:
                S.append("  GatB gp;")
                S.append("  __builtin_memcpy(&gp, (GatBC*)(gb + {}), sizeof(GatB));".format(member))
                S.append("  const AdamP ad = gp.ad;")

        head("k_fwd", self.fwd_threads, "blockIdx.y")
        S.extend(fwd_body)
        head("k_final", "NB", "blockIdx.z")
        S.extend(finals["k_final"][1])
        head("k_loss", 64, "blockIdx.x")
        S.extend(finals["k_loss"][1])
        for gi in range(len(self.gathers)):
            name = "k_gat_{}".format(gi)
            if name not in gathers or "T* __restrict__ g, const AdamP ad" not in gathers[name][0]:
                raise TraceUnsupported("batched gather kernels: gather {} has no pointwise kernel of its own".format(gi))
            head(name, "NB", "blockIdx.y", gat=True)
            S.append("  T* __restrict__ g = gp.g[{}];".format(gi))
            S.extend(gathers[name][1])
        if self.merged:
            if "const GatAll ga" not in gathers["k_gat_all"][0]:
                raise TraceUnsupported("batched gather kernels: the merged gather is not the pointwise kernel")
            head("k_gat_all", "NB", "blockIdx.y", gat=True)
            S.append("  GatAll ga;")
            for k, key in enumerate(self.merged):
                S.append("  ga.g[{0}] = gp.g[{1}]; ga.ad[{0}] = ad;".format(k, self.gathers.index(key)))
            S.extend(gathers["k_gat_all"][1])

    def _par_batch_kernel(self, S, par_lines):
        """`k_par_batch` and `jit_par_batch`: the body of `k_par` (param_expr.emit: its lines as emitted, after the
        signature) for the B members of an ensemble.  `k_par` is ONE workgroup, so the member is blockIdx.x; its `Args`
        and its `ParArgs` (val / grad: its slices of the packed parameters and their gradients, pout: its row of the packed
        terms and norms) are read from DEVICE memory through the constant address space into by-value copies, as the other
        batched kernels read theirs; the host scalars travel in the member's `Args`."""
        body = self._kernel_bodies(par_lines)["k_par"][1]
        S.append("typedef const __attribute__((address_space(4))) ParArgs ParArgsC;")
        S.append('extern "C" __global__ __launch_bounds__(NB) void k_par_batch(const Args* __restrict__ ab, '
                 'const ParArgs* __restrict__ pb) {')
        S.append("  Args a;")
        S.append("  __builtin_memcpy(&a, (ArgsC*)(ab + blockIdx.x), sizeof(Args));")
        S.append("  ParArgs pa;")
        S.append("  __builtin_memcpy(&pa, (ParArgsC*)(pb + blockIdx.x), sizeof(ParArgs));")
        S.extend(body)
        S.append('extern "C" int jit_par_batch(const void* args_dev, const void* pargs_dev, int nmembers, void* stream) {')
        S.append("  if (nmembers < 1 || nmembers > 65535) return -1;")
        S.append("  hipLaunchKernelGGL(k_par_batch, dim3(nmembers), dim3(NB), 0, (hipStream_t)stream, (const Args*)args_dev, "
                 "(const ParArgs*)pargs_dev);")
        S.append("  return (int)hipGetLastError();")
        S.append("}")

    def _epoch_batch_launchers(self, S, nout):
        """`jit_fwd_batch`, `jit_gather_batch` (which = -1: the merged gather): args_dev / ptrs_dev are `nmembers` argument
        blocks / `GatB` back to back in DEVICE memory."""
        S.append('extern "C" int jit_fwd_batch(const void* args_dev, int nmembers, void* stream) {')
        S.append("  if (nmembers < 1 || nmembers > 65535) return -1;")
        S.append("  const Args* ab = (const Args*)args_dev;")
        S.append("  hipLaunchKernelGGL(k_fwd_batch, dim3({}, nmembers), dim3({}), 0, (hipStream_t)stream, ab);".format(
            self.fwd_blocks, self.fwd_threads))
        S.append("  hipLaunchKernelGGL(k_final_batch, dim3({}, SEG, nmembers), dim3(NB), 0, (hipStream_t)stream, ab);".format(
            nout + len(self.pg_decl)))  # (the rows of k_final: the outputs, then the parameter gradients of networks and `Array` unknowns)
        S.append("  hipLaunchKernelGGL(k_loss_batch, dim3(nmembers), dim3(64), 0, (hipStream_t)stream, ab);")
        S.append("  return (int)hipGetLastError();")
        S.append("}")
        S.append('extern "C" int jit_gather_batch(int which, const void* args_dev, const void* ptrs_dev, int nmembers, void* stream) {')
        S.append("  if (nmembers < 1 || nmembers > 65535) return -1;")
        S.append("  const Args* ab = (const Args*)args_dev;")
        S.append("  const GatB* gb = (const GatB*)ptrs_dev;")
        S.append("  switch (which) {")
        for gi, key in enumerate(self.gathers):
            nblk = self.gather_blocks.get(gi, (int(np.prod(self._field_shape(key))) + 255) // 256)
            S.append("    case {0}: hipLaunchKernelGGL(k_gat_{0}_batch, dim3({1}, nmembers), dim3(NB), 0, (hipStream_t)stream, ab, gb); "
                     "break;".format(gi, nblk))
        if self.merged:
            S.append("    case -1: hipLaunchKernelGGL(k_gat_all_batch, dim3({}, nmembers), dim3(NB), 0, (hipStream_t)stream, ab, gb); "
                     "break;".format(self.gather_all_blocks))
        S.append("    default: return -1;")
        S.append("  }")
        S.append("  return (int)hipGetLastError();")
        S.append("}")
