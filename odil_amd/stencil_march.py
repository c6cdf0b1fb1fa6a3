"""The MARCHING form of the forward kernel `k_fwd` of stencil_codegen.py -- network evaluations shared between
neighbouring points (stencil_share.py; float kernels with a pointwise network at the faces) -- with the sums of read
cotangents it forms in the kernel and the final gathers `k_gat_*` that go with them.
"""

import os

import numpy as np

from . import stencil_grad


class _MarchKernels:
    """Methods of `stencil_codegen._Codegen`: chosen by `_choose_shared_calls`, emitted from `source()`."""

    def _march_parts(self):
        """Line groups of the marching forward kernel (see _march_kernel): per variant (general / interior) the forward
        lines before and after the shared network values, and the reverse pass."""
        a1, a2 = self.ndim - 2, self.ndim - 1
        by_axis = {axis: (A, B) for A, B, axis in self.share}
        (Ax, Bx), (Ay, By) = by_axis[a1], by_axis[a2]
        shared = {x.idx for x in (Ax, Bx, Ay, By)}
        late = set()
        for n in self.order:
            if (n.op == "mlp_out" and n.args[0].idx in shared) or any(a.idx in late for a in n.args):
                late.add(n.idx)
        early = {n.idx for n in self.order} - late
        attr = Bx.attr
        nlast = len(attr[2]) - 1
        nz, nin = attr[2][nlast], len(Bx.args)
        parts = dict(Ax=Ax, Bx=Bx, Ay=Ay, By=By, nz=nz, nin=nin, attr=attr, variants=[])
        plan = self._fold_plan(self.order, 1, windows=True)
        # a third copy for the strips that touch a wall of the LANE axis (2 of 9 at 512 columns): predicates of the other
        # axes folded, those of the lane axis kept
        plan_w = self._fold_plan(self.order, 4, windows=True) if plan is not None else None
        if plan_w is not None and (plan_w[0] == plan[0] or a2 not in plan[1]):
            plan_w = None  # (no predicate of the lane axis: the interior copy serves every strip)
        parts["plan"], parts["plan_w"] = plan, plan_w
        # the general variant stores its adjoints as the body of k_fwd; the folded copies must store the same (_body)
        pref = dict()
        for fold in ([None] if plan is None else ([None, plan[0]] + ([plan_w[0]] if plan_w is not None else []))):
            live = None if fold is None else self._live_under(fold)
            with self._body(fold=fold, march_pref=pref, march_live=live, fresh_adjoints=fold is not None) as body:
                self.forward(only=early)
                fwd1 = body.take()
                xin = [(self.r(Bx.args[k]), self.r(By.args[k]), self.r(Ay.args[k])) for k in range(nin)]
                self.forward(only=late)
                fwd2 = body.take()
                self.reverse()
                rev = body.take()
            rev_text = "\n".join(rev)

            def adjoint_of(call, j):
                out = self.mlp_out_seen.get(call.idx, dict()).get(j)
                return "g{}".format(out.idx) if out is not None and "T g{} ".format(out.idx) in rev_text else "(T)0"

            adj = {name: [adjoint_of(call, j) for j in range(nz)] for name, call in (("ax", Ax), ("bx", Bx), ("ay", Ay), ("by", By))}
            parts["variants"].append(dict(fwd1=fwd1, fwd2=fwd2, rev=rev, xin=xin, adj=adj, used=body.march_used))
        parts["pref"] = sorted(pref.values())
        parts["gather"] = self._march_gather_plan()
        # the pre-steps of a row segment: the inputs of the LOWER face along the marching axis at the segment's first row,
        # and of the lower face along the lane axis at the strip's first column
        for tag, call in (("", Ax), ("_y", Ay)):
            seen = dict()
            for arg in call.args:
                for n in stencil_grad.subdag(arg):
                    seen[n.idx] = n
            with self._body(order=[seen[i] for i in sorted(seen)]) as body:
                self.forward()
                parts["pre_lines" + tag], parts["pre_in" + tag] = body.lines, [self.r(arg) for arg in call.args]
        # the packed evaluation (prefix mu) and the reverse pass of the PREVIOUS step's evaluation (prefix mp)
        with self._body() as body:
            self._mlp_forward("mu", 2, attr, [("ux{}_0".format(k), "ux{}_1".format(k)) for k in range(nin)])
            parts["mlp_fwd"] = body.take()
            self._mlp_backward("mp", 2, attr, [("ud{}_0".format(j), "ud{}_1".format(j)) for j in range(nz)], False)
            parts["mlp_bwd"] = body.take()
            self._mlp_backward("mu", 2, attr, [("ud{}_0".format(j), "ud{}_1".format(j)) for j in range(nz)], False)
            parts["mlp_bwd_mu"] = body.take()
        layers = attr[2]
        parts["acts"] = ["h{}_{}".format(l, i) for l in range(nlast) for i in range(layers[l])]  # what the reverse pass reads
        return parts

    def _march_gather_plan(self):
        """The cotangents of the reads of a marching kernel summed IN the kernel over the marching axis (a three-row delay
        line in registers) and over the lane axis (lane shifts) before they are stored: one array per (field, shift on the
        leading axes) instead of one per stencil read -- heat with two space dimensions: 2 instead of 10 (32 bytes per
        point less written by k_fwd and read again by the gather).  What crosses a segment of rows or a strip of columns
        goes to small EDGE arrays which the final gather adds.  None when the reads do not have that shape."""
        if self.cut_nodes or self.jac_store or not self.cots:
            return None
        a1, a2 = self.ndim - 2, self.ndim - 1
        groups = dict()
        for slot, n in enumerate(self.cots):
            key, shift, loc, _ = n.attr
            if not self._regular(n):
                return None
            cs = []
            for d, sh in enumerate(shift):
                ext = self.G[d]
                v = sh % ext
                cs.append(v - ext if v > ext // 2 else v)
            sx, sy = cs[a1], cs[a2]
            if abs(sx) > 1 or abs(sy) > 1 or (sx and sy):
                return None
            groups.setdefault((key, tuple(cs[:a1])), []).append((slot, sx, sy))
        if any(adj is not None for adj in self.out_adj):
            return None
        return dict(groups=list(groups.items()))

    def _march_gather_geometry(self):
        a1, a2 = self.ndim - 2, self.ndim - 1
        G1, G2 = self.G[a1], self.G[a2]
        R = max(1, min(int(os.environ.get("ODIL_TRACE_MARCH_ROWS", 64)), G1, 64))  # (<= 64: one lane of the pre-step per row)
        nseg, nstrip = (G1 + R - 1) // R, (G2 + 63) // 64
        lead = int(np.prod(self.G[:a1])) if a1 > 0 else 1
        return R, nseg, nstrip, lead

    def _march_edge_offsets(self, ngroups):
        """Element offsets into a.edge of the four edge arrays of every group: E_lo, E_hi [lead, nseg, G2] (rows that
        cross a segment), F_lo, F_hi [lead, G1, nstrip] (columns that cross a strip); total size."""
        a1, a2 = self.ndim - 2, self.ndim - 1
        R, nseg, nstrip, lead = self._march_gather_geometry()
        esz, fsz = lead * nseg * self.G[a2], lead * self.G[a1] * nstrip
        offs, o = [], 0
        for _ in range(ngroups):
            offs.append((o, o + esz, o + 2 * esz, o + 2 * esz + fsz))
            o += 2 * esz + 2 * fsz
        return offs, o

    def _march_gather_kernels(self, S, plan):
        """The final gathers of a marching kernel with the in-kernel partial sums (_march_gather_plan): per field
        g[j] = sum over its groups of (P + edge terms)[j - leading shift], four points of the last axis per thread."""
        a1, a2 = self.ndim - 2, self.ndim - 1
        G1, G2 = self.G[a1], self.G[a2]
        R, nseg, nstrip, lead = self._march_gather_geometry()
        groups = plan["groups"]
        offs, _ = self._march_edge_offsets(len(groups))
        vw = 4 if G2 % 4 == 0 else 1
        keys = []
        for (key, _), _ in groups:
            if key not in keys:
                keys.append(key)
        self.gathers, self.direct, self.merged, self.gather_blocks = list(keys), dict(), [], dict()
        self.gather_reads_sources = {key: [] for key in keys}
        for gi, key in enumerate(keys):
            threads = self.total // vw
            self.gather_blocks[gi] = (threads + 255) // 256
            S.append('extern "C" __global__ __launch_bounds__(NB) void k_gat_{}(const Args a, T* __restrict__ g, const AdamP ad) {{'.format(gi))
            S.append("  const int lr = blockIdx.x * NB + threadIdx.x;")
            S.append("  if (lr >= {}) return;".format(threads))
            names = ["i{}".format(d) for d in range(self.ndim)]
            self._index_prologue(S, self.G, names, vw, "lr")
            if vw == 1:
                S.append("  const int ib = i{};".format(a2))
            S.append("  T acc[{}];".format(vw))
            S.append("  for (int p = 0; p < {}; ++p) acc[p] = (T)0;".format(vw))
            S.append("  const int seg = i{} / {};".format(a1, R))
            for k, ((gkey, lshift), _) in enumerate(groups):
                if gkey != key:
                    continue
                e_lo, e_hi, f_lo, f_hi = offs[k]
                S.append("  {")
                # the point this group's sums were formed at: j - leading shift (periodic)
                lidx = []
                for d in range(a1):
                    lidx.append("i{}".format(d) if lshift[d] == 0 else "wrap(i{} - ({}), {})".format(d, lshift[d], self.G[d]))
                lflat = self._offset(lidx, self.G[:a1]) if a1 > 0 else "0"
                S.append("  const int lf = {};".format(lflat))
                S.append("  const T* const P = a.cot[{}] + ((long)lf * {} + i{}) * {};".format(k, G1, a1, G2))
                if vw == 4:
                    S.append("  { const T4 q = *(const T4*)(P + ib); acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w; }")
                else:
                    S.append("  acc[0] += P[ib];")
                # rows that received a contribution from the neighbouring segment
                S.append("  if (i{0} % {1} == {1} - 1 || i{0} == {2}) {{".format(a1, R, G1 - 1))
                S.append("    const T* const E = a.edge + {} + ((long)lf * {} + (seg + 1 == {} ? 0 : seg + 1)) * {};".format(e_lo, nseg, nseg, G2))
                S.append("    for (int p = 0; p < {}; ++p) acc[p] += E[ib + p];".format(vw))
                S.append("  }")
                S.append("  if (i{} % {} == 0) {{".format(a1, R))
                S.append("    const T* const E = a.edge + {} + ((long)lf * {} + (seg == 0 ? {} : seg - 1)) * {};".format(e_hi, nseg, nseg - 1, G2))
                S.append("    for (int p = 0; p < {}; ++p) acc[p] += E[ib + p];".format(vw))
                S.append("  }")
                # columns that received a contribution from the neighbouring strip
                S.append("  for (int p = 0; p < {}; ++p) {{".format(vw))
                S.append("    const int c = ib + p, st = c / 64;")
                S.append("    const T* const F = a.edge + ((long)lf * {} + i{}) * {};".format(G1, a1, nstrip))
                S.append("    if (c % 64 == 63 || c == {}) acc[p] += F[{} + (st + 1 == {} ? 0 : st + 1)];".format(G2 - 1, f_lo, nstrip))
                S.append("    if (c % 64 == 0) acc[p] += F[{} + (st == 0 ? {} : st - 1)];".format(f_hi, nstrip - 1))
                S.append("  }")
                S.append("  }")
            o = "lr * 4" if vw == 4 else "lr"
            if vw == 4:
                if self.nt_streams:
                    S.append("  __builtin_nontemporal_store((T4){{acc[0], acc[1], acc[2], acc[3]}}, (T4*)(g + {}));".format(o))
                else:
                    S.append("  *(T4*)(g + {}) = (T4){{acc[0], acc[1], acc[2], acc[3]}};".format(o))
                S.append("  adam_apply4(ad, {}, acc);".format(o))
            else:
                S.append("  g[{}] = acc[0];".format(o))
                S.append("  adam_apply(ad, {}, acc[0]);".format(o))
            S.append("}")

    def _march_kernel(self, S, parts, stored, stream):
        """Body of the MARCHING forward kernel of an operator that evaluates one pointwise network at the faces of every
        cell (heat with two space dimensions: reference examples/heat/heat.py:86-98 per axis).  The lower face of cell i is
        the upper face of cell i - e (stencil_share.py proves it on the DAG), so half of the evaluations of the plain
        kernel -- and of their reverse passes, two thirds of its instructions -- are repeats.  Here a WAVE owns a strip of
        64 columns of the last axis and marches along the second-to-last axis over a segment of rows; every lane makes ONE
        packed evaluation per point: (upper face along the marching axis, upper face along the lane axis).

        * marching axis: the value of a point's upper face is carried in registers to the next row, where it is the lower
          face; the adjoint it collects there is added to its own before the reverse pass of the evaluation, which
          therefore runs ONE STEP LATE, from the previous step's activations (carried as well);
        * lane axis: lane L takes its lower face from lane L - 1 and returns the adjoint to it by wave-wide lane shifts
          (DPP: no LDS, no barrier);
        * a segment starts with a PRE-STEP whose packed evaluation holds the lower faces nobody hands over: slot 0 the
          marching axis' at the segment's first row (every lane its column), slot 1 the lane axis' at the strip's FIRST
          column -- lane j for row r0 + j (a segment has at most 64 rows).  Lane 0 fetches its row's value with
          v_readlane as the march goes and hands the adjoint back the same way; after the march a post-step repeats the
          pre-step's forward pass from the kept inputs and runs its reverse pass with the collected adjoints.  (Until
          this form a HELPER lane per wave evaluated the first column's lower face every step: 63 columns per wave,
          nine waves per row of 512 where eight suffice.)

        Values and adjoints of lanes without a point are masked; sums of network-parameter gradients are linear in the
        adjoints, so a face shared by two waves (or two segments) simply contributes from both sides.  The body exists
        twice: as traced, and with every index predicate folded to its interior value (_fold_plan); the branch is scalar
        (row index, strip and leading indices are wave-uniform)."""
        a1, a2 = self.ndim - 2, self.ndim - 1
        G1, G2 = self.G[a1], self.G[a2]
        R, nseg, nstrip, lead = self._march_gather_geometry()
        nitems = lead * nseg * nstrip
        nz, nin, attr = parts["nz"], parts["nin"], parts["attr"]
        nl = len(attr[2]) - 1
        Ax, Bx, Ay, By = parts["Ax"], parts["Bx"], parts["Ay"], parts["By"]
        acts = parts["acts"]
        S.append("  const int lane = threadIdx.x & 63;")
        S.append("  const int wave_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);")
        S.append("  for (int item = blockIdx.x * 4 + wave_; item < {}; item += a.nblocks * 4) {{".format(nitems))
        S.append("  const int strip = item % {}, seg = (item / {}) % {};".format(nstrip, nstrip, nseg))
        rem = "(item / {})".format(nstrip * nseg)
        for d in reversed(range(a1)):
            if d == 0:
                S.append("  const int i0 = {};".format(rem))
            else:
                S.append("  const int i{} = {} % {};".format(d, rem, self.G[d]))
                S.append("  const int q{}_ = {} / {};".format(d, rem, self.G[d]))
                rem = "q{}_".format(d)
        S.append("  const int r0 = seg * {0}, r1 = min(r0 + {0}, {1});".format(R, G1))
        S.append("  const int p2 = strip * 64 + lane;")
        S.append("  const bool valid = p2 < {};".format(G2))
        S.append("  const int i{} = min(p2, {});".format(a2, G2 - 1))
        # interior test, scalar: leading indices, strip range; the row is tested per step
        plan, plan_w = parts["plan"], parts.get("plan_w")
        outer, rowc, leadc = [], [], []
        if plan is not None:
            _, exc, _ = plan
            for d, values in sorted(exc.items()):
                if d < a1:
                    outer.append(self._interior_cond({d: values}))
                    leadc.append(outer[-1])
                elif d == a1:
                    rowc.append(self._interior_cond({d: values}))
                else:  # no exceptional column among the strip's: [s0, s0 + 63]
                    values, lo, hi = list(values), 0, G2 - 1
                    while values and values[0] == lo:
                        values.pop(0)
                        lo += 1
                    while values and values[-1] == hi:
                        values.pop()
                        hi -= 1
                    if lo > 0:
                        outer.append("strip * 64 >= {}".format(lo))
                    if hi < G2 - 1:
                        outer.append("strip * 64 + 63 <= {}".format(hi))
                    outer.extend("!(strip * 64 <= {0} && {0} <= strip * 64 + 63)".format(e) for e in values)
            S.append("  const bool interior_ = {};".format(" && ".join(outer) or "true"))
            S.append("  const bool lead_ok_ = {};".format(" && ".join(leadc) or "true"))  # (the wall-strip copy's condition)
        # carried state
        mg = parts["gather"]
        if mg is not None:
            for k in range(len(mg["groups"])):
                S.append("  T ap{0} = (T)0, ac{0} = (T)0;".format(k))  # sums of rows r - 1 and r so far
        for j in range(nz):
            S.append("  T kx{0} = (T)0, gbx{0} = (T)0, gy{0} = (T)0;".format(j))
        for name in acts:
            S.append("  T2 mp_{0} = (T2)(0.0f);".format(name))
        # ---- pre-step: the LOWER faces the march cannot take from a neighbour -- slot 0: along the marching axis at row r0,
        # own column; slot 1: along the lane axis at the strip's FIRST column, lane j for row r0 + j (the strip's lane 0
        # fetches them with v_readlane as the march goes; its adjoints come back the same way and are passed through the
        # network's reverse pass after the march, from a second forward pass over the kept inputs)
        for k in range(nin):
            S.append("  T axin{0}, ayin{0};".format(k))
        S.append("  {")
        S.append("  const int i{} = r0;".format(a1))
        S.extend(parts["pre_lines"])
        for k in range(nin):
            S.append("  axin{} = {};".format(k, parts["pre_in"][k]))
        S.append("  }")
        S.append("  {")
        S.append("  const int i{} = min(r0 + lane, r1 - 1);".format(a1))
        S.append("  const int i{} = min(strip * 64, {});".format(a2, G2 - 1))
        S.extend(parts["pre_lines_y"])
        for k in range(nin):
            S.append("  ayin{} = {};".format(k, parts["pre_in_y"][k]))
        S.append("  }")
        for j in range(nz):
            S.append("  T kay{0}, gedge{0} = (T)0;".format(j))
        S.append("  {")
        for k in range(nin):
            S.append("  const T ux{0}_0 = axin{0}, ux{0}_1 = ayin{0};".format(k))
        S.extend(parts["mlp_fwd"])
        for j in range(nz):
            S.append("  kx{0} = mu_z{1}_{0}.x; kay{0} = mu_z{1}_{0}.y;".format(j, nl))
        for name in acts:
            S.append("  mp_{0} = mu_{0};".format(name))
        S.append("  }")
        # ---- the march ----------------------------------------------------------------------------------------------
        # the field values a step reads are requested during the step before (the step's arithmetic covers their
        # latency: two resident waves per SIMD cannot)
        pref = parts["pref"]
        if pref:
            S.append("  T {};".format(", ".join("ldn_{}".format(k) for k, _ in pref)))
            S.append("  {{ const int i{} = r0;".format(a1))
            for k, e in pref:
                S.append("    ldn_{} = {};".format(k, e))
            S.append("  }")
        S.append("  for (int i{0} = r0; i{0} < r1; ++i{0}) {{".format(a1))
        S.append("  const int l = {};".format(self._offset(["i{}".format(d) for d in range(self.ndim)], self.G)))
        if pref:
            for k, _ in pref:
                S.append("  const T ld_{0} = ldn_{0};".format(k))
            S.append("  {{ const int inext_ = min(i{0} + 1, r1 - 1); {{ const int i{0} = inext_;".format(a1))
            vs = parts["variants"]
            row = " && ".join(rowc) or "true"
            always = vs[1]["used"] if len(vs) > 1 else {k for k, _ in pref}
            wall = (vs[2]["used"] | always) if len(vs) > 2 else None
            for k, e in pref:
                if k in always:
                    S.append("    ldn_{} = {};".format(k, e))
            if wall is not None and len(wall) > len(always):  # what the wall-strip copy reads beyond the interior one
                S.append("    if (!(interior_ && {})) {{".format(row))
                for k, e in pref:
                    if k in wall and k not in always:
                        S.append("      ldn_{} = {};".format(k, e))
                S.append("    }")
            rest = [(k, e) for k, e in pref if k not in (wall if wall is not None else always)]
            if rest:  # what only the general copy of the body reads: when the next row takes that copy
                S.append("    if (!({} && {})) {{".format("lead_ok_" if wall is not None else "interior_", row))
                for k, e in rest:
                    S.append("      ldn_{} = {};".format(k, e))
                S.append("    }")
            S.append("  } }")
        for j in range(nz):
            S.append("  T gax{0}, gbc{0}, gay{0}, gby{0}, zx{0};".format(j))
        for name in acts:
            S.append("  T2 mc_{};".format(name))
        if mg is not None:
            for k in range(len(mg["groups"])):
                S.append("  T cm{0}, c0{0}, cp{0}, yl{0}, yr{0};".format(k))

        mg = parts["gather"]

        def body(var, inbox):
            B = []
            B.extend(self._inbox_lines(inbox))
            B.extend(var["fwd1"])
            for k, (bx, by, ay) in enumerate(var["xin"]):
                B.append("  const T ux{0}_0 = {1}, ux{0}_1 = {2};".format(k, bx, by))
            B.extend(parts["mlp_fwd"])
            for name in acts:
                B.append("  mc_{0} = mu_{0};".format(name))
            for j in range(nz):
                z = "mu_z{}_{}".format(nl, j)
                B.append("  const T m{}_z{}_{} = kx{};".format(Ax.idx, nl, j, j))
                B.append("  const T m{}_z{}_{} = {}.x;".format(Bx.idx, nl, j, z))
                B.append("  const T m{}_z{}_{} = {}.y;".format(By.idx, nl, j, z))
                # (two statements: a lane shift inside one arm of a conditional would run with lane 0 masked off, and a DPP
                # read from a disabled lane is invalid -- lane 1 would get 0)
                B.append("  const T ayp{0}_ = odil_lane_prev({1}.y), ay0{0}_ = odil_readlane(kay{0}, i{2} - r0);".format(j, z, a1))
                B.append("  const T m{0}_z{1}_{2} = lane == 0 ? ay0{2}_ : ayp{2}_;".format(Ay.idx, nl, j))
                B.append("  zx{} = {}.x;".format(j, z))
            B.extend(var["fwd2"])
            B.extend(var["rev"])
            if mg is not None:
                # partial sums of the read cotangents (_march_gather_plan): per group what this row gives to the rows
                # r - 1, r, r + 1 (cm, c0, cp; c0 with the lane neighbours' shares) and to the neighbouring strips
                for k, (_, members) in enumerate(mg["groups"]):
                    gsum = lambda sel: " + ".join("g{}".format(self.cots[slot].idx) for slot, sx, sy in members if sel(sx, sy)) or None
                    term = lambda e: "(valid ? {} : (T)0)".format(e) if e else None
                    c0, cm, cp = gsum(lambda sx, sy: sx == 0 and sy == 0), gsum(lambda sx, sy: sx == -1), gsum(lambda sx, sy: sx == 1)
                    yl, yr = gsum(lambda sx, sy: sy == -1), gsum(lambda sx, sy: sy == 1)  # to the column left / right
                    B.append("  cm{} = {};".format(k, term(cm) or "(T)0"))
                    B.append("  cp{} = {};".format(k, term(cp) or "(T)0"))
                    B.append("  yl{} = {};".format(k, term(yl) or "(T)0"))
                    B.append("  yr{} = {};".format(k, term(yr) or "(T)0"))
                    B.append("  c0{} = {};".format(k, term(c0) or "(T)0"))
            B.append("  if (valid) {")
            for slot, (n, name) in enumerate(stored if mg is None else []):
                if stream:
                    B.append("    __builtin_nontemporal_store({}, &a.cot[{}][l]);".format(name, slot))
                else:
                    B.append("    a.cot[{}][l] = {};".format(slot, name))
            for k, (o_, raw) in enumerate(zip(self.outputs, self.raw)):
                term = self.r(o_) if raw else "{0} * {0}".format(self.r(o_))
                if self.out_lens[k] is not None:
                    term = "(inbox{} ? {} : (T)0)".format(k, term)
                B.append("    s_{0} = s_{0} + {1};".format(k, term))
            B.append("  }")
            for j in range(nz):
                B.append("  gax{0} = valid ? {1} : (T)0; gbc{0} = valid ? {2} : (T)0;".format(j, var["adj"]["ax"][j], var["adj"]["bx"][j]))
                B.append("  gay{0} = valid ? {1} : (T)0; gby{0} = valid ? {2} : (T)0;".format(j, var["adj"]["ay"][j], var["adj"]["by"][j]))
            return B

        variants = parts["variants"]
        if len(variants) == 1:
            S.extend(body(variants[0], ()))
        else:
            S.append("  if (interior_ && {}) {{".format(" && ".join(rowc) or "true"))
            S.extend(body(variants[1], plan[2]))
            if len(variants) > 2:
                S.append("  }} else if (lead_ok_ && {}) {{".format(" && ".join(rowc) or "true"))
                S.extend(body(variants[2], plan_w[2]))
            S.append("  } else {")
            S.extend(body(variants[0], ()))
            S.append("  }")
        if mg is not None:
            offs, _ = self._march_edge_offsets(len(mg["groups"]))
            lead_flat = self._offset(["i{}".format(d) for d in range(a1)], self.G[:a1]) if a1 > 0 else "0"
            S.append("  const long lf_ = {};".format(lead_flat))
            S.append("  const int lastl_ = min(63, {} - strip * 64);".format(G2 - 1))  # the strip's last lane with a point
            for k in range(len(mg["groups"])):
                e_lo, e_hi, f_lo, f_hi = offs[k]
                # the row's own sum: the lane neighbours' shares arrive by lane shifts; what leaves the strip goes to F
                S.append("  const T fromr{0} = odil_lane_next(yl{0}), froml{0} = odil_lane_prev(yr{0});".format(k))
                S.append("  const T row{0} = c0{0} + (valid ? froml{0} + fromr{0} : (T)0);".format(k))
                S.append("  if (lane == 0) a.edge[{} + (lf_ * {} + i{}) * {} + strip] = yl{};".format(f_lo, G1, a1, nstrip, k))
                S.append("  if (lane == lastl_) a.edge[{} + (lf_ * {} + i{}) * {} + strip] = yr{};".format(f_hi, G1, a1, nstrip, k))
                # delay line along the marching axis: row r - 1 is complete (within the segment) once row r has given its share
                S.append("  if (i{} > r0) {{ if (valid) {}; }}".format(
                    a1, ("__builtin_nontemporal_store(ap{0} + cm{0}, &a.cot[{0}][l - {1}])" if stream else "a.cot[{0}][l - {1}] = ap{0} + cm{0}").format(k, G2)))
                S.append("  else if (valid) a.edge[{} + (lf_ * {} + seg) * {} + i{}] = cm{};".format(e_lo, nseg, G2, a2, k))
                S.append("  ap{0} = ac{0} + row{0}; ac{0} = cp{0};".format(k))
        for j in range(nz):  # what lane 0 found for the strip's first lower face of this row: back to the lane that evaluated it
            S.append("  {{ const T g0_ = odil_readlane(gay{0}, 0); gedge{0} = lane == i{1} - r0 ? g0_ : gedge{0}; }}".format(j, a1))
        # reverse pass of the PREVIOUS step's evaluation: its own adjoints + what this row found for the carried face
        S.append("  {")
        for j in range(nz):
            S.append("  const T ud{0}_0 = gbx{0} + gax{0}, ud{0}_1 = gy{0};".format(j))
        S.extend(parts["mlp_bwd"])
        S.append("  }")
        for j in range(nz):
            S.append("  kx{0} = zx{0}; gbx{0} = gbc{0}; gy{0} = gby{0} + odil_lane_next(gay{0});".format(j))
        for name in acts:
            S.append("  mp_{0} = mc_{0};".format(name))
        S.append("  }")  # rows
        if mg is not None:
            # the segment's last row (what the next segment's first row gives it arrives through E_lo), and what the last
            # row gives to the next segment's first row
            offs, _ = self._march_edge_offsets(len(mg["groups"]))
            lead_flat = self._offset(["i{}".format(d) for d in range(a1)], self.G[:a1]) if a1 > 0 else "0"
            S.append("  if (valid) {")
            S.append("    const long lf_ = {};".format(lead_flat))
            last_l = self._offset(["i{}".format(d) if d != a1 else "(r1 - 1)" for d in range(self.ndim)], self.G)
            S.append("    const int ll_ = {};".format(last_l))
            for k in range(len(mg["groups"])):
                e_lo, e_hi, f_lo, f_hi = offs[k]
                S.append("    a.cot[{0}][ll_] = ap{0};".format(k))
                S.append("    a.edge[{} + (lf_ * {} + seg) * {} + i{}] = ac{};".format(e_hi, nseg, G2, a2, k))
            S.append("  }")
        # flush: the last row's evaluation (its upper face along the marching axis belongs to the next segment too)
        S.append("  {")
        for j in range(nz):
            S.append("  const T ud{0}_0 = gbx{0}, ud{0}_1 = gy{0};".format(j))
        S.extend(parts["mlp_bwd"])
        S.append("  }")
        # post-step: the reverse pass of the pre-step's second slot (the lane axis' lower faces of the first column)
        S.append("  {")
        for k in range(nin):
            S.append("  const T ux{0}_0 = axin{0}, ux{0}_1 = ayin{0};".format(k))
        S.extend(parts["mlp_fwd"])
        for j in range(nz):
            S.append("  const T ud{0}_0 = (T)0, ud{0}_1 = lane < r1 - r0 ? gedge{0} : (T)0;".format(j))
        S.append("  {")
        S.extend(parts["mlp_bwd_mu"])
        S.append("  }")
        S.append("  }")
        S.append("  }")  # items
