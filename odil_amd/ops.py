"""Tensor-level wrappers of the HIP kernels (torch = device memory + streams only).

Each function allocates its output with torch, passes raw device pointers through
the C-ABI (`_lib.call`) on the current HIP stream and returns tensors.  Names and
semantics follow the reference functions cited in include/odil_hip.h.
"""

import math
from ctypes import c_double, c_int, c_int32, c_int64, c_size_t, c_void_p

import torch

from . import _lib
from ._lib import call, host_reals, i64, ptr, ptr_array, stream_ptr

_workspace = {}


def reduce_workspace(device, nquant=1):
    """Per-device scratch for the deterministic reductions (f64 partial sums)."""
    key = (str(device), nquant)
    ws = _workspace.get(key)
    if ws is None:
        ws = torch.empty(_lib.reduce_workspace_elems() * nquant, dtype=torch.float64, device=device)
        _workspace[key] = ws
    return ws


_column_sums = {}


def residual_synth_workspace(device, cshape):
    """Per-device scratch of poisson_residual_synth (f64 sums of squares per coarse column and z-chunk): allocated once,
    replaced only by a larger one."""
    need = _lib.load().odil_poisson_residual_synth_workspace_bytes(i64(cshape)) // 8
    ws = _column_sums.get(str(device))
    if ws is None or ws.numel() < need:
        ws = _column_sums[str(device)] = torch.empty(max(need, 1), dtype=torch.float64, device=device)
    return ws


def fine_shape(cshape, loc):
    return tuple({"c": 2 * s, "n": 2 * s - 1, ".": s}[l] for s, l in zip(cshape, loc))


def coarse_shape(fshape, loc):
    """Output shape of restrict_to_coarser (stride-2 VALID on every axis)."""
    return tuple((s - 2) // 2 + 1 if l == "c" else (s - 1) // 2 + 1 for s, l in zip(fshape, loc))


def _lead_stride(t):
    """The leading stride of a 4-D view that is contiguous but for that stride (a level array of the slab paths without
    its outer ghost planes), else None."""
    if t.dim() != 4 or t.is_contiguous() or t.shape[0] < 2:
        return None
    inner = t[0]
    return int(t.stride(0)) if inner.is_contiguous() and t.stride(0) >= inner.numel() else None


def interp_add(coarse, loc, add=None, coarse_scale=1.0, add_scale=1.0, out=None):
    """out = add_scale*add + P(coarse_scale*coarse)  (reference core.py:606-700, :258-262).  `coarse` may be a 4-D view
    with a leading stride larger than its volume: the marching kernels read it in place, other layouts get a copy."""
    fshape = fine_shape(coarse.shape, loc)
    if out is None:
        out = torch.empty(fshape, dtype=coarse.dtype, device=coarse.device)
    assert tuple(out.shape) == fshape, (out.shape, fshape)
    if add is not None:
        assert tuple(add.shape) == fshape and add.dtype == coarse.dtype
    if not coarse.is_contiguous():
        ld = _lead_stride(coarse)
        if ld is not None and call(
            "interp_add_ld", coarse.dtype, c_void_p(coarse.data_ptr()), c_int64(ld), ptr(add), ptr(out), i64(coarse.shape),
            c_int(coarse.dim()), loc.encode(), coarse_scale, add_scale, stream_ptr(), unserved_ok=True,
        ):
            return out
        coarse = coarse.contiguous()
    call(
        "interp_add", coarse.dtype, ptr(coarse), ptr(add), ptr(out), i64(coarse.shape), c_int(coarse.dim()),
        loc.encode(), coarse_scale, add_scale, stream_ptr(),
    )
    return out


def interp_to_finer(u, loc, depth=1):
    for _ in range(depth):
        u = interp_add(u, loc)
    return u


def interp_adj(gfine, loc, cshape, scale=None, out=None, cut=(False, False)):
    """P^T gfine (and optionally scale * P^T gfine).  cut=(lo, hi): axis 0 is an interior slab
    interface at that end (ghost planes), not a wall."""
    cshape = tuple(int(s) for s in cshape)
    assert tuple(gfine.shape) == fine_shape(cshape, loc), (gfine.shape, cshape, loc)
    if out is None:
        out = torch.empty(cshape, dtype=gfine.dtype, device=gfine.device)
    if not out.is_contiguous():
        # a view with a leading stride larger than its volume is written in place where the kernels can; else through
        # a contiguous result
        assert scale is None and not any(cut), "a strided result takes no scaled copy and no cut"
        ld = _lead_stride(out)
        if ld is None or not call("interp_adj_ld", gfine.dtype, ptr(gfine), c_void_p(out.data_ptr()), c_int64(ld), i64(cshape),
                                  c_int(len(cshape)), loc.encode(), stream_ptr(), unserved_ok=True):
            out.copy_(interp_adj(gfine, loc, cshape))
        return out
    scaled = None
    if scale is not None:
        scaled = torch.empty_like(out)
    call(
        "interp_adj_cut", gfine.dtype, ptr(gfine), ptr(out), ptr(scaled), i64(cshape), c_int(len(cshape)),
        loc.encode(), 1.0 if scale is None else float(scale), c_int(1 if cut[0] else 0), c_int(1 if cut[1] else 0),
        stream_ptr(),
    )
    return out if scale is None else (out, scaled)


def _step_size(alpha, dtype):
    """(host value, device pointer or None): `alpha` may be a one-element device tensor -- the step size
    is then read from memory by the kernel (an epoch captured into a hipGraph replays with new values)."""
    if isinstance(alpha, torch.Tensor):
        assert alpha.numel() == 1 and alpha.dtype == dtype
        return 0.0, ptr(alpha)
    return float(alpha), None


def interp_adj_adam(gfine, loc, cshape, out, x, m, v, alpha, one_minus_b1, one_minus_b2, eps, cut=(False, False)):
    """out = P^T gfine and the Adam step of (x, m, v) (arrays of out's shape) with that gradient."""
    cshape = tuple(int(s) for s in cshape)
    assert tuple(out.shape) == cshape == tuple(x.shape) == tuple(m.shape) == tuple(v.shape)
    a, adev = _step_size(alpha, gfine.dtype)
    call(
        "interp_adj_cut_adam", gfine.dtype, ptr(gfine), ptr(out), i64(cshape), c_int(len(cshape)), loc.encode(),
        c_int(1 if cut[0] else 0), c_int(1 if cut[1] else 0), ptr(x), ptr(m), ptr(v), a,
        float(one_minus_b1), float(one_minus_b2), float(eps), adev, stream_ptr(),
    )
    return out


def restrict_to_coarser(u, loc, depth=1):
    """Full weighting (reference core.py:703-755)."""
    for _ in range(depth):
        out = torch.empty(coarse_shape(u.shape, loc), dtype=u.dtype, device=u.device)
        call("restrict", u.dtype, ptr(u), ptr(out), i64(u.shape), c_int(u.dim()), loc.encode(), stream_ptr())
        u = out
    return u


def conv_valid(x, w, strides, transposed=False, out_shape=None):
    """Strided VALID correlation of `x` with the small dense kernel `w` (same rank), or its transpose (see
    include/odil_hip.h: odil_conv_valid).  `out_shape` only for the transpose: a longer output than (n - 1) s + K."""
    dim = x.dim()
    strides = [int(s) for s in strides]
    assert w.dim() == dim and len(strides) == dim and w.dtype == x.dtype
    if transposed:
        oshape = [(n - 1) * s + k for n, s, k in zip(x.shape, strides, w.shape)]
        if out_shape is not None:
            assert all(a >= b for a, b in zip(out_shape, oshape)), (out_shape, oshape)
            oshape = [int(v) for v in out_shape]
    else:
        oshape = [(n - k) // s + 1 for n, s, k in zip(x.shape, strides, w.shape)]
    out = torch.empty(oshape, dtype=x.dtype, device=x.device)
    call("conv_valid", x.dtype, ptr(x), ptr(w), ptr(out), i64(x.shape), i64(w.shape), i64(strides), i64(oshape), c_int(dim),
         c_int(1 if transposed else 0), stream_ptr())
    return out


def stencil_var_smooth(coeffs, x, b, omega, out):
    """out = x - omega (A x - b) / c0 for the (2 d + 1)-point operator with coefficient arrays `coeffs` [(2 d + 1), *shape]
    (include/odil_hip.h: odil_stencil_var_smooth, mode 0).  x = None: from the zero vector (x' = omega b / c0: two words)."""
    assert coeffs.shape[0] == 2 * b.dim() + 1 and tuple(coeffs.shape[1:]) == tuple(b.shape) == tuple(out.shape) and out is not x
    call("stencil_var_smooth", b.dtype, ptr(coeffs), ptr(x), ptr(b), ptr(out), i64(b.shape), c_int(b.dim()), float(omega),
         c_int(0), stream_ptr())
    return out


def smooth2_supported(shape):
    return 1 <= len(shape) <= 3 and shape[-1] % 2 == 0 and min(shape) >= 2


def stencil_var_smooth2(coeffs, x, b, omega1, omega2, out, zc_hint=0):
    """Two sweeps of `stencil_var_smooth` (weights omega1, then omega2) in ONE pass over the coefficient arrays;
    bit-identical to two calls (out is not x).  x = None: from the zero vector (x is not read)."""
    assert coeffs.shape[0] == 2 * b.dim() + 1 and tuple(coeffs.shape[1:]) == tuple(b.shape) == tuple(out.shape)
    assert x is None or (x.shape == b.shape and out.data_ptr() != x.data_ptr() and x.is_contiguous())
    assert smooth2_supported(tuple(b.shape)) and coeffs.is_contiguous() and b.is_contiguous()
    call("stencil_var_smooth2", b.dtype, ptr(coeffs), ptr(x), ptr(b), ptr(out), i64(b.shape), c_int(b.dim()), float(omega1),
         float(omega2), c_int(zc_hint), stream_ptr())
    return out


def stencil_var_residual(coeffs, x, b, out=None):
    """b - A x (mode 1 of odil_stencil_var_smooth)."""
    assert coeffs.shape[0] == 2 * x.dim() + 1 and tuple(coeffs.shape[1:]) == tuple(x.shape)
    out = torch.empty_like(x) if out is None else out
    call("stencil_var_smooth", x.dtype, ptr(coeffs), ptr(x), ptr(b), ptr(out), i64(x.shape), c_int(x.dim()), 0.0, c_int(1),
         stream_ptr())
    return out


def stencil_var_residual_restrict(coeffs, x, b, scale, out, loss, zrange=None, denom=0.0):
    """out = scale * (sum over the 2^d children of b - A x), loss <- mean((A x - b)^2), one pass.  zrange = (z0, z1): the
    slab form -- loss = sum over those planes of (A x - b)^2 / denom."""
    assert tuple(out.shape) == tuple(s // 2 for s in x.shape) and out.is_contiguous()
    if zrange is None:  # (loss = None: no reduction launch)
        call("stencil_var_residual_restrict", x.dtype, ptr(coeffs), ptr(x), ptr(b), ptr(out), i64(x.shape), c_int(x.dim()),
             float(scale), ptr(reduce_workspace(x.device)), ptr(loss), stream_ptr())
    else:
        call("stencil_var_residual_restrict_slab", x.dtype, ptr(coeffs), ptr(x), ptr(b), ptr(out), i64(x.shape),
             c_int(x.dim()), float(scale), c_int64(int(zrange[0])), c_int64(int(zrange[1])), c_double(float(denom)),
             ptr(reduce_workspace(x.device)), ptr(loss), stream_ptr())
    return out


def narrow_scale(x64, y32, a=1.0, msq=None):
    """y32 = (a / sqrt(msq)) * x64 in one pass (msq: 0-d float64 device tensor or None)."""
    assert x64.dtype == torch.float64 and y32.dtype == torch.float32 and x64.numel() == y32.numel()
    lib = _lib.load()
    status = lib.odil_narrow_scale(ptr(x64), ptr(y32), c_int64(x64.numel()), float(a), ptr(msq), stream_ptr())
    if status != 0:
        raise _lib.OdilHipError("odil_narrow_scale: {}".format(lib.odil_last_error().decode()))
    return y32


def widen_axpy(y64, x32, a=1.0, msq=None):
    """y64 += (a * sqrt(msq)) * x32 in one pass."""
    assert y64.dtype == torch.float64 and x32.dtype == torch.float32 and y64.numel() == x32.numel()
    lib = _lib.load()
    status = lib.odil_widen_axpy(ptr(y64), ptr(x32), c_int64(y64.numel()), float(a), ptr(msq), stream_ptr())
    if status != 0:
        raise _lib.OdilHipError("odil_widen_axpy: {}".format(lib.odil_last_error().decode()))
    return y64


def max_abs_diff(a, b):
    """2-element device tensor (max |a - b|, max |b|), one pass over both arrays."""
    assert a.numel() == b.numel() and a.dtype == b.dtype
    out = torch.empty(2, dtype=a.dtype, device=a.device)
    call("max_abs_diff", a.dtype, ptr(a), ptr(b), c_int64(a.numel()), ptr(reduce_workspace(a.device)), ptr(out), stream_ptr())
    return out


def max_abs_rows(a):
    """max |row| of every row of a 2-D view (<= 64 rows) as a device tensor: two launches for all rows."""
    a2 = a.reshape(a.shape[0], -1)
    assert a2.is_contiguous() and 1 <= a2.shape[0] <= 64
    out = torch.empty(a2.shape[0], dtype=a.dtype, device=a.device)
    call("max_abs_rows", a.dtype, ptr(a2), c_int(a2.shape[0]), c_int64(a2.shape[1]), ptr(reduce_workspace(a.device)), ptr(out),
         stream_ptr())
    return out


def stencil_var_coarsen(coeffs, halve=None):
    """Coefficient arrays of the coarse-grid operator [(2 d + 1), *(shape / 2)] (csrc/stencil_mg.hip).  halve: per axis,
    whether two cells are merged along it (default: every axis); the others keep their extent (semi-coarsening)."""
    import ctypes

    shape = tuple(coeffs.shape[1:])
    halve = [True] * len(shape) if halve is None else [bool(h) for h in halve]
    out = torch.empty((coeffs.shape[0],) + tuple(s // 2 if h else s for s, h in zip(shape, halve)), dtype=coeffs.dtype,
                      device=coeffs.device)
    if all(halve):
        call("stencil_var_coarsen", coeffs.dtype, ptr(coeffs), ptr(out), i64(shape), c_int(len(shape)), stream_ptr())
    else:
        mask = (ctypes.c_int * len(shape))(*[int(h) for h in halve])
        call("stencil_var_coarsen_axes", coeffs.dtype, ptr(coeffs), ptr(out), i64(shape), c_int(len(shape)),
             ctypes.cast(mask, ctypes.c_void_p), stream_ptr())
    return out


def _packed_members(t, need):
    """(pointer, member stride in elements) of a packed tensor [B, >= need] with contiguous members (any leading stride)."""
    assert t.dim() == 2 and t.shape[1] >= need and (t.shape[1] == 1 or t.stride(1) == 1), (tuple(t.shape), need)
    return _base_ptr(t), c_int64(int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]))


def stencil_var_coarsen_batch(coeffs, shape, halve=None, out=None):
    """`stencil_var_coarsen` for every member of an ensemble in ONE launch (include/odil_hip.h:
    odil_stencil_var_coarsen_batch).  coeffs: [B, >= (2 d + 1) cells], member b's arrays of `shape` at the start of row b;
    out: [B, >= (2 d + 1) coarse cells] likewise (default: a new tensor without padding).  Rows may be views into wider
    buffers (the levels of one packed hierarchy)."""
    import ctypes

    shape = tuple(int(n) for n in shape)
    ndim, nb = len(shape), coeffs.shape[0]
    halve = [True] * ndim if halve is None else [bool(h) for h in halve]
    cshape = tuple(n // 2 if h else n for n, h in zip(shape, halve))
    if out is None:
        out = torch.empty((nb, (2 * ndim + 1) * math.prod(cshape)), dtype=coeffs.dtype, device=coeffs.device)
    assert out.shape[0] == nb and out.dtype == coeffs.dtype
    cp, cs = _packed_members(coeffs, (2 * ndim + 1) * math.prod(shape))
    op, os_ = _packed_members(out, (2 * ndim + 1) * math.prod(cshape))
    mask = (ctypes.c_int * ndim)(*[int(h) for h in halve])
    call("stencil_var_coarsen_batch", coeffs.dtype, cp, cs, op, os_, i64(shape), c_int(ndim),
         ctypes.cast(mask, ctypes.c_void_p), c_int(nb), stream_ptr())
    return out


def stencil_strength_batch(coeffs, shape, out=None):
    """[B, 2 d]: max |c| of every off-centre coefficient array of every member in ONE launch -- `max_abs_rows(c[1:])` per
    member (odil_stencil_strength_batch).  coeffs as in `stencil_var_coarsen_batch`."""
    shape = tuple(int(n) for n in shape)
    ndim, nb = len(shape), coeffs.shape[0]
    if out is None:
        out = torch.empty((nb, 2 * ndim), dtype=coeffs.dtype, device=coeffs.device)
    assert tuple(out.shape) == (nb, 2 * ndim) and out.dtype == coeffs.dtype
    cp, cs = _packed_members(coeffs, (2 * ndim + 1) * math.prod(shape))
    call("stencil_strength_batch", coeffs.dtype, cp, cs, i64(shape), c_int(ndim), c_int(nb), ptr(out), stream_ptr())
    return out


def stencil_dense_batch(coeffs, shape, out=None):
    """[B, n, n]: the dense matrix of every member's operator (n = cells <= 512, column j = A e_j with periodic wrap) in ONE
    launch (odil_stencil_dense_batch).  coeffs as in `stencil_var_coarsen_batch`."""
    shape = tuple(int(n) for n in shape)
    ndim, nb, n = len(shape), coeffs.shape[0], math.prod(shape)
    if out is None:
        out = torch.empty((nb, n, n), dtype=coeffs.dtype, device=coeffs.device)
    assert tuple(out.shape) == (nb, n, n) and out.dtype == coeffs.dtype
    cp, cs = _packed_members(coeffs, (2 * ndim + 1) * n)
    call("stencil_dense_batch", coeffs.dtype, cp, cs, i64(shape), c_int(ndim), c_int(nb), ptr(out), stream_ptr())
    return out


def stencil_var_smooth_batch_parts(shape):
    """Partial sums per member that `stencil_var_smooth_batch` writes for members of `shape` (0: malformed shape)."""
    return int(_lib.load().odil_stencil_var_smooth_batch_parts(i64(shape), c_int(len(shape))))


def _active_ptr(active, nb):
    if active is not None:
        assert active.dtype == torch.int32 and tuple(active.shape) == (nb,) and active.is_contiguous()
    return ptr(active)


def stencil_var_smooth_batch(coeffs, x, b, omega, out, mode=0, active=None, partials=None):
    """`stencil_var_smooth` (mode 0; x = None: from the zero vector) or `stencil_var_residual` (mode 1) for every member of
    an ensemble in ONE launch (include/odil_hip.h: odil_stencil_var_smooth_batch).  coeffs: [B, >= (2 d + 1) cells] as in
    `stencil_var_coarsen_batch`; x, b, out: [B, *shape] with contiguous members (any leading stride), out is not x.
    active: None or int32 [B], members with a zero are skipped whole.  partials (mode 0): None or float64 [B, P], P =
    `stencil_var_smooth_batch_parts(shape)`: per workgroup the sum of (A x - b)^2 of the sweep's input."""
    nb, shape = b.shape[0], tuple(int(n) for n in b.shape[1:])
    ndim, cells = len(shape), math.prod(shape)
    assert tuple(out.shape) == tuple(b.shape) and out.dtype == b.dtype == coeffs.dtype and coeffs.shape[0] == nb
    assert x is None or (tuple(x.shape) == tuple(b.shape) and x.dtype == b.dtype)
    if partials is not None:
        assert partials.dtype == torch.float64 and partials.is_contiguous()
        assert tuple(partials.shape) == (nb, stencil_var_smooth_batch_parts(shape)), tuple(partials.shape)
    cp, cs = _packed_members(coeffs, (2 * ndim + 1) * cells)
    call("stencil_var_smooth_batch", b.dtype, cp, cs, None if x is None else _base_ptr(x),
         c_int64(0 if x is None else _member_stride(x, cells)), _base_ptr(b), c_int64(_member_stride(b, cells)), _base_ptr(out),
         c_int64(_member_stride(out, cells)), i64(shape), c_int(ndim), c_int(nb), float(omega), c_int(mode),
         _active_ptr(active, nb), ptr(partials), stream_ptr())
    return out


def stencil_var_smooth2_batch(coeffs, x, b, omega1, omega2, out, active=None, zc_hint=0):
    """`stencil_var_smooth2` (two sweeps, weights omega1 then omega2, in ONE pass over the coefficient arrays; x = None:
    from the zero vector) for every member of an ensemble in ONE launch (include/odil_hip.h:
    odil_stencil_var_smooth2_batch): per member the bits of two `stencil_var_smooth` calls.  Arrays, strides and `active`
    as in `stencil_var_smooth_batch`, members of a shape `smooth2_supported` admits, every member on a pack boundary
    (even strides); out is not x."""
    nb, shape = b.shape[0], tuple(int(n) for n in b.shape[1:])
    ndim, cells = len(shape), math.prod(shape)
    assert smooth2_supported(shape), shape
    assert tuple(out.shape) == tuple(b.shape) and out.dtype == b.dtype == coeffs.dtype and coeffs.shape[0] == nb
    assert x is None or (tuple(x.shape) == tuple(b.shape) and x.dtype == b.dtype)
    pack = 2 * b.element_size()
    assert all(t is None or t.data_ptr() % pack == 0 for t in (coeffs, x, b, out)), "arrays must begin on a pack boundary"
    cp, cs = _packed_members(coeffs, (2 * ndim + 1) * cells)
    call("stencil_var_smooth2_batch", b.dtype, cp, cs, None if x is None else _base_ptr(x),
         c_int64(0 if x is None else _member_stride(x, cells)), _base_ptr(b), c_int64(_member_stride(b, cells)), _base_ptr(out),
         c_int64(_member_stride(out, cells)), i64(shape), c_int(ndim), c_int(nb), float(omega1), float(omega2), c_int(zc_hint),
         _active_ptr(active, nb), stream_ptr())
    return out


def stencil_var_residual_restrict_batch(coeffs, x, b, scale, out, active=None):
    """out = scale * (sum over the 2^d children of b - A x) for every member in ONE launch (odil_stencil_var_residual_
    restrict_batch): every axis merged, even extents, no norm.  Arrays as in `stencil_var_smooth_batch`; out: [B, *shape / 2]."""
    nb, shape = x.shape[0], tuple(int(n) for n in x.shape[1:])
    ndim, cells = len(shape), math.prod(shape)
    assert tuple(out.shape) == (nb,) + tuple(n // 2 for n in shape) and tuple(b.shape) == tuple(x.shape)
    assert out.dtype == b.dtype == x.dtype == coeffs.dtype and coeffs.shape[0] == nb
    cp, cs = _packed_members(coeffs, (2 * ndim + 1) * cells)
    call("stencil_var_residual_restrict_batch", x.dtype, cp, cs, _base_ptr(x), c_int64(_member_stride(x, cells)), _base_ptr(b),
         c_int64(_member_stride(b, cells)), _base_ptr(out), c_int64(_member_stride(out, cells // 2**ndim)), i64(shape),
         c_int(ndim), c_int(nb), float(scale), _active_ptr(active, nb), stream_ptr())
    return out


def stencil_cycle_decide_batch(partials, cells, k, maxcycles, tol, history, outcome, active, nactive, partials0=None):
    """The decision of every active member before cycle k (odil_stencil_cycle_decide_batch): history[b, 1 + k] from the
    member's partial sums [B, P] (history[b, 0] from partials0 when given), the stop rules of `stencil_solve_batch`,
    outcome [B, 2] and active [B] (int32) updated for the members that stop, the members still active counted into nactive
    (int32, one element).  Everything stays on the device."""
    nb = partials.shape[0]
    assert partials.dtype == torch.float64 and partials.dim() == 2 and partials.is_contiguous()
    assert partials0 is None or (partials0.dtype == torch.float64 and partials0.shape == partials.shape
                                 and partials0.is_contiguous())
    assert history.dtype == torch.float64 and history.shape[0] == nb and history.is_contiguous()
    assert outcome.dtype == torch.int32 and tuple(outcome.shape) == (nb, 2) and outcome.is_contiguous()
    assert nactive.dtype == torch.int32 and nactive.numel() == 1
    lib = _lib.load()
    status = lib.odil_stencil_cycle_decide_batch(
        ptr(partials), c_int64(partials.shape[1]), ptr(partials0), c_int64(partials.shape[1]), c_int(partials.shape[1]),
        c_int(nb), c_int64(int(cells)), c_int(k), c_int(maxcycles), c_double(float(tol)), ptr(history),
        c_int64(history.shape[1]), ptr(outcome), _active_ptr(active, nb), ptr(nactive), stream_ptr())
    if status != 0:
        raise _lib.OdilHipError("odil_stencil_cycle_decide_batch: {}".format(lib.odil_last_error().decode()))
    return nactive


def stencil_gcr_batch_parts(cells):
    """Partial sums per member and quantity that the `stencil_gcr_*_batch` passes leave (0: cells outside 1..2^24)."""
    return int(_lib.load().odil_stencil_gcr_batch_parts(c_int64(int(cells))))


class GcrBatch:
    """The device state and the launches of GCR(m) for an ensemble in lock-step (include/odil_hip.h:
    odil_stencil_gcr_*_batch), allocated once: store [B, 2 m, cells] (Z, then Q), rho [B, *shape], zero [B, *shape]
    (never written: the right-hand side of t = 0 - A e), the masks active / gcr / fresh / verify and have (int32 [B]),
    scal [B, m + 2], gpart [B, m + 2, P], counts (int32 [4]) with a pinned host copy.  Everything a pass reads about a
    member comes from these device arrays."""

    def __init__(self, nbatch, shape, m, dtype, device, active):
        self.nb, self.shape, self.m, self.dtype = int(nbatch), tuple(int(n) for n in shape), int(m), dtype
        self.cells = math.prod(self.shape)
        self.parts = stencil_gcr_batch_parts(self.cells)
        if not self.parts or not 1 <= self.m <= 8:
            raise ValueError("GcrBatch: {} cells per member, {} directions (1..2^24 cells, 1..8 directions)".format(self.cells, m))
        self.store = torch.zeros((self.nb, 2 * self.m, self.cells), dtype=dtype, device=device)
        self.rho = torch.zeros((self.nb,) + self.shape, dtype=dtype, device=device)
        self.zero = torch.zeros((self.nb,) + self.shape, dtype=dtype, device=device)
        self.active = active
        self.flags = torch.zeros((4, self.nb), dtype=torch.int32, device=device)
        self.gcr, self.fresh, self.verify, self.have = self.flags[0], self.flags[1], self.flags[2], self.flags[3]
        self.scal = torch.zeros((self.nb, self.m + 2), dtype=torch.float64, device=device)
        self.gpart = torch.zeros((self.nb, self.m + 2, self.parts), dtype=torch.float64, device=device)
        self.counts = torch.zeros(4, dtype=torch.int32, device=device)
        self.counts_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self._common = (c_int64(self.cells), c_int(self.m))
        self._gp = (ptr(self.gpart), c_int64((self.m + 2) * self.parts))
        self._sc = (ptr(self.scal), c_int64(self.m + 2))
        self._st = (ptr(self.store), c_int64(2 * self.m * self.cells))

    def row(self, r):
        """[B, *shape]: row r of every member's store (a strided view: contiguous members)."""
        return self.store[:, r].unflatten(1, self.shape)

    def reset(self):
        self.flags.zero_()

    def dots(self, slot):
        call("stencil_gcr_dots_batch", self.dtype, *self._st, *self._common, c_int(slot), ptr(self.have), c_int(self.m),
             ptr(self.gcr), c_int(self.nb), *self._gp, stream_ptr())

    def project(self, slot):
        call("stencil_gcr_project_batch", self.dtype, *self._st, ptr(self.rho), c_int64(self.cells), *self._common, c_int(slot),
             ptr(self.have), c_int(self.m), *self._sc, ptr(self.gcr), c_int(self.nb), *self._gp, stream_ptr())

    def update(self, slot, x):
        call("stencil_gcr_update_batch", self.dtype, *self._st, _base_ptr(x), c_int64(_member_stride(x, self.cells)),
             ptr(self.rho), c_int64(self.cells), *self._common, c_int(slot), *self._sc, ptr(self.gcr), c_int(self.nb),
             *self._gp, stream_ptr())

    def sumsq(self, v, mask):
        call("stencil_gcr_sumsq_batch", self.dtype, _base_ptr(v), c_int64(_member_stride(v, self.cells)), c_int64(self.cells),
             ptr(mask), c_int(self.nb), *self._gp, stream_ptr())

    def decide(self, mode, k, maxcycles, tol, history, outcome, partials, partials0=None):
        """odil_stencil_gcr_decide_batch; after the modes 0 and 3 `counts` holds the members of every kind."""
        assert history.dtype == torch.float64 and history.shape[0] == self.nb and history.is_contiguous()
        assert outcome.dtype == torch.int32 and tuple(outcome.shape) == (self.nb, 3) and outcome.is_contiguous()
        assert partials.dtype == torch.float64 and partials.dim() == 2 and partials.is_contiguous()
        assert partials0 is None or (partials0.shape == partials.shape and partials0.is_contiguous())
        lib = _lib.load()
        status = lib.odil_stencil_gcr_decide_batch(
            c_int(mode), ptr(partials), c_int64(partials.shape[1]), ptr(partials0), c_int64(partials.shape[1]),
            c_int(partials.shape[1]), self._gp[0], self._gp[1], c_int(self.parts), c_int(self.nb), c_int64(self.cells), c_int(k),
            c_int(maxcycles), c_double(float(tol)), c_int(self.m), ptr(history), c_int64(history.shape[1]), ptr(outcome),
            ptr(self.active), ptr(self.gcr), ptr(self.fresh), ptr(self.verify), ptr(self.have), self._sc[0], self._sc[1],
            ptr(self.counts), stream_ptr())
        if status != 0:
            raise _lib.OdilHipError("odil_stencil_gcr_decide_batch: {}".format(lib.odil_last_error().decode()))


def stencil_vcycle_tail(coeffs, shapes, halve, xin, b, xout, work, inv, wpre, wpost, fmg=False):
    """The coarse tail of a multigrid cycle in one launch (include/odil_hip.h: odil_stencil_vcycle_tail).  coeffs: one
    flat tensor holding the coefficient arrays of every tail level; shapes: their extents, finest first; halve: per
    transition and axis, whether cell pairs are merged; xin None: zero start."""
    import ctypes

    nlev, ndim = len(shapes), len(shapes[0])
    flat = [int(n) for shape in shapes for n in shape]
    mask = (ctypes.c_int * max(1, (nlev - 1) * ndim))(*[int(bool(h)) for tr in halve for h in tr])
    wa, wap = host_reals(list(wpre) or [0.0], b.dtype)
    wb, wbp = host_reals(list(wpost) or [0.0], b.dtype)
    call("stencil_vcycle_tail", b.dtype, ptr(coeffs), i64(flat), ctypes.cast(mask, ctypes.c_void_p), c_int(nlev), c_int(ndim),
         ptr(xin), ptr(b), ptr(xout), ptr(work), ctypes.c_int64(work.numel()), ptr(inv), c_int(inv.shape[0]), wap,
         c_int(len(wpre)), wbp, c_int(len(wpost)), c_int(1 if fmg else 0), stream_ptr())
    return xout


def stencil_vcycle_tail_plan(coeffs, shapes, halve, work, inv, wpre, wpost):
    """`stencil_vcycle_tail` with everything that does not change between calls prepared once (a cycle visits its tail
    every 0.3 ms: building the argument arrays anew cost ~30 us of host time per visit, which the GPU waited for right
    after each cycle's read-back): -> launch(xin, b, xout, fmg)."""
    import ctypes

    nlev, ndim = len(shapes), len(shapes[0])
    shapes64 = i64([int(n) for shape in shapes for n in shape])
    mask = (ctypes.c_int * max(1, (nlev - 1) * ndim))(*[int(bool(h)) for tr in halve for h in tr])
    maskp = ctypes.cast(mask, ctypes.c_void_p)
    wa, wap = host_reals(list(wpre) or [0.0], coeffs.dtype)
    wb, wbp = host_reals(list(wpost) or [0.0], coeffs.dtype)
    fixed = (ptr(coeffs), shapes64, maskp, c_int(nlev), c_int(ndim))
    rest = (ptr(work), ctypes.c_int64(work.numel()), ptr(inv), c_int(inv.shape[0]), wap, c_int(len(wpre)), wbp, c_int(len(wpost)))
    keep = (coeffs, work, inv, mask, wa, wb, shapes64)  # (the arrays the pointers point into)
    dtype = coeffs.dtype

    def launch(xin, b, xout, fmg=False):
        call("stencil_vcycle_tail", dtype, *fixed, ptr(xin), ptr(b), ptr(xout), *rest, c_int(1 if fmg else 0), stream_ptr())
        return xout

    launch.keep = keep
    return launch


def stencil_solve_batch_work(shapes):
    """Work elements per member of `stencil_solve_batch` (0: malformed shapes)."""
    flat = [int(n) for shape in shapes for n in shape]
    return int(_lib.load().odil_stencil_solve_batch_work(i64(flat), c_int(len(shapes)), c_int(len(shapes[0]))))


def stencil_solve_krylov_batch_work(shapes, m):
    """Work elements per member of `stencil_solve_krylov_batch_plan` with m directions: `stencil_solve_batch_work` plus
    (2 m + 2) finest-level vectors (0: malformed shapes, or m outside 1..8)."""
    flat = [int(n) for shape in shapes for n in shape]
    return int(_lib.load().odil_stencil_solve_krylov_batch_work(i64(flat), c_int(len(shapes)), c_int(len(shapes[0])),
                                                                 c_int(int(m))))


def _member_stride(t, need, shared_ok=False):
    """Elements between the members of a packed tensor [B, ...] whose members are contiguous (0: one member shared by all)."""
    if shared_ok and t.dim() == 1:
        return 0
    assert t.dim() >= 2 and t[0].is_contiguous() and t[0].numel() >= need, (tuple(t.shape), need)
    return int(t.stride(0)) if t.shape[0] > 1 else int(t[0].numel())


def _base_ptr(t):
    """Device pointer of the first element of a packed tensor (its members are contiguous, the whole need not be)."""
    if not t.is_cuda:
        raise _lib.OdilHipError("tensor is on '{}': the HIP kernels need device memory (no CPU fallback)".format(t.device))
    return c_void_p(t.data_ptr())


def stencil_solve_batch_plan(coeffs, shapes, halve, nbatch, work, inv, wpre, wpost, krylov_m=None):
    """`stencil_solve_batch` with everything that does not change between calls prepared once (as
    `stencil_vcycle_tail_plan`): -> launch(x, b, history, outcome, start, mode, maxcycles, tol).
    coeffs: flat [ncoeff] (one operator for all members) or [B, ncoeff]; inv: [n, n] or [B, n, n]; work: [B, >= need];
    x, b: [B, *shape] with contiguous members (any leading stride); history: [B, >= maxcycles + 2] float64; outcome:
    [B, 2] int32.  krylov_m: `stencil_solve_krylov_batch_plan`."""
    import ctypes

    nlev, ndim = len(shapes), len(shapes[0])
    cells, ninv = math.prod(shapes[0]), math.prod(shapes[-1])
    shapes64 = i64([int(n) for shape in shapes for n in shape])
    mask = (ctypes.c_int * max(1, (nlev - 1) * ndim))(*[int(bool(h)) for tr in halve for h in tr])
    maskp = ctypes.cast(mask, ctypes.c_void_p)
    wa, wap = host_reals(list(wpre) or [0.0], coeffs.dtype)
    wb, wbp = host_reals(list(wpost) or [0.0], coeffs.dtype)
    need = stencil_solve_batch_work(shapes) if krylov_m is None else stencil_solve_krylov_batch_work(shapes, krylov_m)
    ncoeff = (2 * ndim + 1) * sum(math.prod(s) for s in shapes)
    cstride = _member_stride(coeffs, ncoeff, shared_ok=True)
    istride = 0 if inv.dim() == 2 else _member_stride(inv, ninv * ninv)
    wstride = _member_stride(work, need)
    assert work.shape[0] == nbatch and work.is_contiguous() and coeffs.dtype == work.dtype == inv.dtype
    # (coeffs [B, ncoeff] may be columns of a wider buffer -- the tail of a hierarchy whose finer levels run as launches)
    assert (coeffs.is_contiguous() if cstride == 0 else coeffs.dim() == 2) and inv.is_contiguous()
    assert tuple(inv.shape[-2:]) == (ninv, ninv)
    assert (coeffs.numel() >= ncoeff if cstride == 0 else coeffs.shape[0] == nbatch) and (istride == 0 or inv.shape[0] == nbatch)
    head = (_base_ptr(coeffs), c_int64(cstride), shapes64, maskp, c_int(nlev), c_int(ndim), c_int(nbatch))
    mid = (ptr(work), c_int64(wstride), c_int64(work.numel()), _base_ptr(inv), c_int64(istride), c_int(ninv), wap,
           c_int(len(wpre)), wbp, c_int(len(wpost)))
    keep = (coeffs, work, inv, mask, wa, wb, shapes64)  # (the arrays the pointers point into)
    dtype = coeffs.dtype
    entry, columns = ("stencil_solve_batch", 2) if krylov_m is None else ("stencil_solve_krylov_batch", 3)
    tail = () if krylov_m is None else (c_int(int(krylov_m)),)

    def launch(x, b, history, outcome, start=2, mode=0, maxcycles=60, tol=0.0):
        assert x.dtype == b.dtype == dtype and x.shape[0] == b.shape[0] == nbatch
        assert history.dtype == torch.float64 and history.shape[0] == nbatch and history.is_contiguous()
        assert outcome.dtype == torch.int32 and tuple(outcome.shape) == (nbatch, columns) and outcome.is_contiguous()
        call(entry, dtype, *head, _base_ptr(x), c_int64(_member_stride(x, cells)),
             _base_ptr(b), c_int64(_member_stride(b, cells)), *mid, c_int(start), c_int(mode), c_int(maxcycles),
             float(tol), ptr(history), c_int64(history.shape[1]), ptr(outcome), *tail, stream_ptr())
        return x

    launch.keep = keep
    return launch


def stencil_solve_krylov_batch_plan(coeffs, shapes, halve, nbatch, work, inv, wpre, wpost, m=6):
    """`stencil_solve_batch_plan` for odil_stencil_solve_krylov_batch: a member whose cycles stop contracting goes on with
    GCR(m) around the same cycle inside the launch.  work: [B, >= stencil_solve_krylov_batch_work(shapes, m)]; outcome:
    [B, 3] int32 (passes, stop reason -- 4: breakdown of GCR --, the cycle of the hand-over or -1)."""
    if not 1 <= int(m) <= 8:
        raise ValueError("stencil_solve_krylov_batch_plan: m = {} (1..8 directions)".format(m))
    return stencil_solve_batch_plan(coeffs, shapes, halve, nbatch, work, inv, wpre, wpost, krylov_m=int(m))


def stencil_solve_batch(coeffs, shapes, halve, x, b, work, inv, wpre, wpost, history, outcome, start=2, mode=0, maxcycles=60,
                        tol=0.0):
    """Whole multigrid solves (mode 1: Newton steps) of x.shape[0] small systems in ONE launch, one workgroup per member
    (include/odil_hip.h: odil_stencil_solve_batch); the arguments of `stencil_solve_batch_plan`."""
    return stencil_solve_batch_plan(coeffs, shapes, halve, x.shape[0], work, inv, wpre, wpost)(
        x, b, history, outcome, start, mode, maxcycles, tol)


def restrict_adj(gcoarse, loc, fshape):
    """R^T gcoarse (cotangent of restrict_to_coarser) for a fine array of shape `fshape`."""
    fshape = tuple(int(s) for s in fshape)
    assert tuple(gcoarse.shape) == coarse_shape(fshape, loc), (gcoarse.shape, fshape, loc)
    out = torch.empty(fshape, dtype=gcoarse.dtype, device=gcoarse.device)
    call("restrict_adj", gcoarse.dtype, ptr(gcoarse), ptr(out), i64(fshape), c_int(len(fshape)), loc.encode(),
         stream_ptr())
    return out


def _shapes_flat(tensors):
    flat = []
    for t in tensors:
        flat += list(t.shape)
    return i64(flat)


def mg_synth(terms, loc, factors=None, work=None, out=None):
    """u = sum_l P^l (f_l w_l)  (reference core.py:245-263)."""
    nlvl = len(terms)
    dtype, device = terms[0].dtype, terms[0].device
    if out is None:
        out = torch.empty_like(terms[0])
    if work is None:
        work = [None] + [torch.empty_like(t) for t in terms[1:-1]] + [None]
        work = work[:nlvl]
    fac = host_reals(factors, dtype) if factors is not None else (None, None)
    call(
        "mg_synth", dtype, ptr_array(terms), fac[1], ptr_array(work), ptr(out), _shapes_flat(terms), c_int(nlvl),
        c_int(terms[0].dim()), loc.encode(), stream_ptr(),
    )
    return out


def _two_step_adjoint(gu, shapes, loc, nontrivial):
    return (gu.dim() == 4 and loc == "nccc" and len(shapes) >= 2 and not nontrivial
            and gu.numel() * gu.element_size() >= (64 << 20) and all(s % 2 == 0 for s in gu.shape[1:]))


def interp_adj_best(gfine, loc, cshape, out=None):
    """P^T of ONE level through the fastest route for the layout: large 'nccc' arrays as space part ('.ccc', batched
    march kernel) then time part ('n...'), as mg_synth_adj does for its first level; interp_adj otherwise."""
    cshape = tuple(int(s) for s in cshape)
    if _two_step_adjoint(gfine, [tuple(gfine.shape), cshape], loc, False):
        space = interp_adj(gfine, "." + loc[1:], (gfine.shape[0],) + cshape[1:])
        return interp_adj(space, "n...", cshape, out=out)
    return interp_adj(gfine, loc, cshape, out=out)


def mg_synth_adj(gu, shapes, loc, factors=None, grads=None):
    """[f_l (P^T)^l gu]  (cotangent of mg_synth)."""
    nlvl = len(shapes)
    dtype, device = gu.dtype, gu.device
    nontrivial = factors is not None and any(float(f) != 1.0 for f in factors)
    if _two_step_adjoint(gu, shapes, loc, nontrivial):
        # 4-D space-time layout 'nccc', large: P^T of the first (dominant) level as the product of
        # its space part (the batched 'ccc' march kernel, every fine value read ONCE) and its time
        # part (a stream over an array 8x smaller).  The one-kernel version holds three windows of
        # plane sums per thread and re-reads the odd fine volumes (0.5 TB/s in float); the joint
        # ghost rule couples cell axes only, so the transpose factorises exactly over the node axis.
        if grads is None:
            grads = [gu] + [torch.empty(tuple(s), dtype=dtype, device=device) for s in shapes[1:]]
        elif grads[0].data_ptr() != gu.data_ptr():
            grads[0].copy_(gu)
        space = interp_adj(gu, "." + loc[1:], (gu.shape[0],) + tuple(shapes[1][1:]))
        interp_adj(space, "n...", tuple(shapes[1]), out=grads[1])
        if nlvl > 2:
            mg_synth_adj(grads[1], shapes[1:], loc, grads=grads[1:])
        return grads
    if grads is None:
        first = torch.empty_like(gu) if (nontrivial and float(factors[0]) != 1.0) else gu
        grads = [first] + [torch.empty(tuple(s), dtype=dtype, device=device) for s in shapes[1:]]
    work = [None] * nlvl
    if nontrivial:
        work = [None] + [torch.empty(tuple(s), dtype=dtype, device=device) for s in shapes[1:]]
    fac = host_reals(factors, dtype) if factors is not None else (None, None)
    flat = []
    for s in shapes:
        flat += list(s)
    call(
        "mg_synth_adj", dtype, ptr(gu), ptr_array(grads), fac[1], ptr_array(work), i64(flat), c_int(nlvl),
        c_int(gu.dim()), loc.encode(), stream_ptr(),
    )
    return grads


def mg_synth_adj_adam(gu, shapes, loc, grads, x, m, v, alpha, one_minus_b1, one_minus_b2, eps):
    """P^T chain with the Adam update of levels >= 1 inside the launches that form their
    gradients (factors == 1).  x, m, v: level arrays (entry 0 is left alone)."""
    nlvl = len(shapes)
    flat = []
    for s in shapes:
        flat += list(s)
    none0 = lambda arrs: ptr_array([None] + list(arrs[1:]))
    a, adev = _step_size(alpha, gu.dtype)
    call(
        "mg_synth_adj_adam", gu.dtype, ptr(gu), ptr_array(grads), None, ptr_array([None] * nlvl), i64(flat),
        c_int(nlvl), c_int(gu.dim()), loc.encode(), none0(x), none0(m), none0(v), a, float(one_minus_b1),
        float(one_minus_b2), float(eps), adev, stream_ptr(),
    )
    return grads


def field_gather(src, field_loc, shift=None, loc=None):
    """Context.field access (reference core.py:955-969): pad, periodic roll, trim."""
    loc = loc or field_loc
    ndim = src.dim()
    shift = tuple(shift) if shift else (0,) * ndim
    oshape = tuple(
        s + (1 if (lf == "c" and l == "n") else 0) - (1 if (lf == "n" and l == "c") else 0)
        for s, lf, l in zip(src.shape, field_loc, loc)
    )
    out = torch.empty(oshape, dtype=src.dtype, device=src.device)
    call(
        "field_gather", src.dtype, ptr(src), ptr(out), i64(src.shape), c_int(ndim), field_loc.encode(), loc.encode(),
        i64(shift), stream_ptr(),
    )
    return out


def field_scatter(g, src_shape, field_loc, shift=None, loc=None, out=None):
    """Transpose of field_gather; accumulates into `out` if given."""
    loc = loc or field_loc
    ndim = len(src_shape)
    shift = tuple(shift) if shift else (0,) * ndim
    accumulate = out is not None
    if out is None:
        out = torch.empty(tuple(src_shape), dtype=g.dtype, device=g.device)
    call(
        "field_scatter", g.dtype, ptr(g), ptr(out), i64(src_shape), c_int(ndim), field_loc.encode(), loc.encode(),
        i64(shift), c_int(1 if accumulate else 0), stream_ptr(),
    )
    return out


def mean_reduce(x, square=True, out=None):
    """mean(x**2) or mean(x) as a 0-d device tensor, deterministic (reference core.py:1093)."""
    x = x.contiguous()
    if out is None:
        out = torch.empty((), dtype=x.dtype, device=x.device)
    call(
        "mean_reduce", x.dtype, ptr(x), c_int64(x.numel()), c_int(1 if square else 0),
        ptr(reduce_workspace(x.device)), ptr(out), stream_ptr(),
    )
    return out


def poisson_residual(u, rhs, h2, fu=None, loss=None, want_fu=True, zrange=None, denom=None):
    """fu = Lap(u) - rhs with zero-Dirichlet ghosts, loss = mean(fu**2)
    (reference examples/poisson/poisson.py:89-113, core.py:1093).  zrange=(z0, z1) / denom: slab
    variant, loss = sum over planes z0 <= z < z1 of fu^2 / denom."""
    assert u.shape == rhs.shape and u.dtype == rhs.dtype
    if fu is None and want_fu:
        fu = torch.empty_like(u)
    if loss is None:
        loss = torch.empty((), dtype=u.dtype, device=u.device)
    h2a, h2p = host_reals(h2, u.dtype)
    if zrange is None:
        call(
            "poisson_residual", u.dtype, ptr(u), ptr(rhs), ptr(fu), i64(u.shape), c_int(u.dim()), h2p,
            ptr(reduce_workspace(u.device)), ptr(loss), stream_ptr(),
        )
    else:
        call(
            "poisson_residual_slab", u.dtype, ptr(u), ptr(rhs), ptr(fu), i64(u.shape), c_int(u.dim()), h2p,
            c_int64(zrange[0]), c_int64(zrange[1]), c_double(float(denom)), ptr(reduce_workspace(u.device)), ptr(loss),
            stream_ptr(),
        )
    return fu, loss


def residual_restrict_supported(shape, dtype):
    pack = 2 if dtype == torch.float64 else 4
    return len(shape) == 3 and shape[0] % 2 == 0 and shape[1] % 2 == 0 and shape[2] % pack == 0 and min(shape) >= 2


def poisson_residual_restrict(u, rhs, h2, scale, out, loss, zrange=None, denom=0.0):
    """out = scale * (sum over 2x2x2 fine cells of (A u - rhs)) on the next coarser grid, loss = mean((A u -
    rhs)**2), in one pass over u and rhs (3-D; see residual_restrict_supported).  zrange = (z0, z1): the slab form --
    loss = sum over those planes of (A u - rhs)**2 / denom."""
    assert u.shape == rhs.shape and tuple(out.shape) == tuple(n // 2 for n in u.shape)
    assert residual_restrict_supported(tuple(u.shape), u.dtype) and out.is_contiguous()
    h2a, h2p = host_reals(h2, u.dtype)
    if zrange is None:  # (loss = None: no reduction launch)
        call("poisson_residual_restrict", u.dtype, ptr(u), ptr(rhs), ptr(out), i64(u.shape), c_int(3), h2p, float(scale),
             ptr(reduce_workspace(u.device)), ptr(loss) if loss is not None else None, stream_ptr())
    else:
        call("poisson_residual_restrict_slab", u.dtype, ptr(u), ptr(rhs), ptr(out), i64(u.shape), c_int(3), h2p,
             float(scale), c_int64(int(zrange[0])), c_int64(int(zrange[1])), c_double(float(denom)),
             ptr(reduce_workspace(u.device)), ptr(loss), stream_ptr())
    return out, loss


def poisson_jacobi(u, rhs, h2, omega, out):
    """out = u - omega (A u - rhs) / diag(A): one damped-Jacobi sweep of the Poisson stencil (out is not u).
    u = None: the sweep starts from the zero vector (nothing is read for it, nothing need be zeroed)."""
    assert rhs.shape == out.shape and (u is None or (u.shape == rhs.shape and out.data_ptr() != u.data_ptr()))
    h2a, h2p = host_reals(h2, rhs.dtype)
    call("poisson_jacobi", rhs.dtype, ptr(u) if u is not None else None, ptr(rhs), ptr(out), i64(rhs.shape),
         c_int(rhs.dim()), h2p, float(omega), stream_ptr())
    return out


def poisson_small_epochs(x, m, v, g, u, fu, rhs, shapes, h2, alphas, omb1, omb2, eps, losses, norms):
    """alphas.numel() whole epochs of the 1-D / 2-D multigrid Poisson problem in one launch (include/odil_hip.h:
    odil_poisson_small_epochs).  x, m, v, g, u: packed flat vectors of all levels; alphas, losses, norms: device tensors."""
    flat = [int(n) for shape in shapes for n in shape]
    h2a, h2p = host_reals(h2, x.dtype)
    call("poisson_small_epochs", x.dtype, ptr(x), ptr(m), ptr(v), ptr(g), ptr(u), ptr(fu), ptr(rhs), i64(flat),
         c_int(len(shapes)), c_int(len(shapes[0])), h2p, ptr(alphas), c_int(alphas.numel()), float(omb1), float(omb2),
         float(eps), ptr(losses), ptr(norms), ptr(reduce_workspace(x.device)), stream_ptr())
    return losses


def poisson_small_epochs_batch(x, m, v, g, u, fu, rhs, shapes, h2, alphas, omb1, omb2, eps, losses, norms, partials):
    """losses.shape[1] whole epochs of B small multigrid Poisson problems in ONE launch, one workgroup per member
    (include/odil_hip.h: odil_poisson_small_epochs_batch).  x, m, v, g, u: [B, unknowns]; fu, rhs: [B, cells]; losses,
    norms: [B, E]; alphas: [B, E], or [E] shared by all members; partials: [B, n] float64 reduction workspace.  Rows are
    contiguous; the row strides are the member strides."""
    nb, nep = int(losses.shape[0]), int(losses.shape[1])
    for t in (x, m, v, g, u):
        assert t.dim() == 2 and t.shape[0] == nb and t.stride(1) == 1 and t.stride(0) == x.stride(0) and t.dtype == x.dtype
    for t in (fu, rhs):
        assert t.shape[0] == nb and t.is_contiguous() and t.dtype == x.dtype
    assert norms.shape == losses.shape and norms.stride() == losses.stride() and losses.stride(1) == 1
    assert alphas.shape[-1] == nep and alphas.stride(-1) == 1 and (alphas.dim() == 1 or alphas.shape[0] == nb)
    assert partials.dtype == torch.float64 and partials.shape[0] == nb and partials.stride(1) == 1
    flat = [int(n) for shape in shapes for n in shape]
    h2a, h2p = host_reals(h2, x.dtype)
    dev = lambda t: c_void_p(t.data_ptr()) if t.is_cuda else ptr(t)  # (ptr refuses host memory; strided rows are fine here)
    call("poisson_small_epochs_batch", x.dtype, dev(x), dev(m), dev(v), dev(g), dev(u), ptr(fu), ptr(rhs), c_int(nb),
         c_int64(x.stride(0)), c_int64(fu[0].numel()), i64(flat), c_int(len(shapes)), c_int(len(shapes[0])), h2p,
         dev(alphas), c_int64(alphas.stride(0) if alphas.dim() == 2 else 0), c_int(nep), float(omb1), float(omb2),
         float(eps), dev(losses), dev(norms), c_int64(losses.stride(0)), dev(partials), c_int64(partials.stride(0)),
         stream_ptr())
    return losses


def poisson_batch_partials(shape, dtype):
    """Doubles of reduction workspace one member of `poisson_residual_batch` needs (0: not a 1-D / 2-D shape it takes)."""
    return int(_lib.load().odil_poisson_batch_partials(i64(shape), c_int(len(shape)), 8 if dtype == torch.float64 else 4))


def _members(t, nb, shape):
    """(device pointer, member stride in elements) of a [B, *shape] tensor whose members are contiguous."""
    assert t.shape[0] == nb and tuple(t.shape[1:]) == tuple(shape) and t[0].is_contiguous(), (t.shape, t.stride())
    if not t.is_cuda:
        raise _lib.OdilHipError("tensor is on '{}': the HIP kernels need device memory (no CPU fallback)".format(t.device))
    return c_void_p(t.data_ptr()), c_int64(t.stride(0) if nb > 1 else max(t.stride(0), t[0].numel()))


def poisson_residual_batch(u, rhs, h2, fu, loss, partials):
    """fu[b] = Lap(u[b]) - rhs[b] and loss[b] = mean(fu[b]**2) for the B members of [B, *shape] arrays in ONE launch (+ one
    reduction launch); member b computes what `poisson_residual` computes for it alone, bit for bit.  The leading
    strides are the member strides; partials: [B, >= poisson_batch_partials] float64; loss: [B] contiguous."""
    nb, shape = int(u.shape[0]), tuple(u.shape[1:])
    assert u.dtype == rhs.dtype == fu.dtype == loss.dtype and loss.shape == (nb,)
    assert partials.dtype == torch.float64 and partials.dim() == 2 and partials.shape[0] == nb and partials.stride(1) == 1
    (up, us), (rp, rs), (fp, fs) = _members(u, nb, shape), _members(rhs, nb, shape), _members(fu, nb, shape)
    h2a, h2p = host_reals(h2, u.dtype)
    plen = (nb - 1) * partials.stride(0) + partials.shape[1]
    call("poisson_residual_batch", u.dtype, up, rp, fp, c_int(nb), us, rs, fs, i64(shape), c_int(len(shape)), h2p,
         c_void_p(partials.data_ptr()), c_int64(max(partials.stride(0), partials.shape[1])), c_int64(plen), ptr(loss),
         stream_ptr())
    return fu, loss


def poisson_adjoint_adam_batch(fu, h2, scale, out, x, m, v, alphas, one_minus_b1, one_minus_b2, eps):
    """`poisson_adjoint_adam` for the B members of [B, *shape] arrays in ONE launch.  alphas: DEVICE step sizes, [B] (one
    per member) or one element (shared); out = None: the gradient is not stored."""
    nb, shape = int(fu.shape[0]), tuple(fu.shape[1:])
    assert alphas.dtype == fu.dtype and alphas.is_cuda and alphas.numel() in (1, nb) and alphas.is_contiguous()
    (fp, fs), (xp, xs), (mp, ms), (vp, vs) = (_members(t, nb, shape) for t in (fu, x, m, v))
    gp, gs = _members(out, nb, shape) if out is not None else (None, fs)
    h2a, h2p = host_reals(h2, fu.dtype)
    call("poisson_adjoint_adam_batch", fu.dtype, fp, gp, xp, mp, vp, c_int(nb), fs, gs, xs, ms, vs, i64(shape),
         c_int(len(shape)), h2p, float(scale), float(one_minus_b1), float(one_minus_b2), float(eps), ptr(alphas),
         c_int64(1 if alphas.numel() == nb and nb > 1 else 0), stream_ptr())
    return out


def residual_synth_batch_workspace(cshape):
    """(float64 column sums, float64 partial sums) ONE member of `poisson_residual_synth_batch` needs, in elements; (0, 0):
    not a coarse shape it takes."""
    lib = _lib.load()
    return (int(lib.odil_poisson_residual_synth_batch_workspace_bytes(i64(cshape))) // 8,
            int(lib.odil_poisson_residual_synth_batch_partials(i64(cshape))))


def poisson_residual_synth_batch(coarse, w0, rhs, h2, fu, loss, partials, sums):
    """`poisson_residual_synth` for the B members of [B, *shape] arrays in ONE launch (+ the loss replay and the final
    reduction, one launch each): fu[b] = Lap(w0[b] + P coarse[b]) - rhs[b], loss[b] = mean(fu[b]**2), bit for bit what the
    single form computes for member b alone.  coarse: contiguous [B, *cshape]; the leading strides of w0, rhs, fu are the
    member strides; partials: [B, >= partial sums of a member] float64; sums: [B, >= column sums of a member] float64
    contiguous (residual_synth_batch_workspace); loss: [B] contiguous."""
    nb, cshape, shape = int(w0.shape[0]), tuple(coarse.shape[1:]), tuple(w0.shape[1:])
    assert coarse.is_contiguous() and coarse.shape[0] == nb and shape == tuple(2 * s for s in cshape)
    assert coarse.dtype == w0.dtype == rhs.dtype == fu.dtype == loss.dtype and loss.shape == (nb,) and loss.is_contiguous()
    assert partials.dtype == torch.float64 and partials.dim() == 2 and partials.shape[0] == nb and partials.stride(1) == 1
    assert sums.dtype == torch.float64 and sums.dim() == 2 and sums.shape[0] == nb and sums.is_contiguous()
    (wp, ws), (rp, rs), (fp, fs) = _members(w0, nb, shape), _members(rhs, nb, shape), _members(fu, nb, shape)
    h2a, h2p = host_reals(h2, w0.dtype)
    plen = (nb - 1) * partials.stride(0) + partials.shape[1]
    call("poisson_residual_synth_batch", w0.dtype, ptr(coarse), wp, rp, fp, c_int(nb), ws, rs, fs, i64(cshape),
         c_int(len(cshape)), h2p, c_void_p(partials.data_ptr()), c_int64(max(partials.stride(0), partials.shape[1])),
         c_int64(plen), ptr(sums), c_size_t(sums.numel() * 8), ptr(loss), stream_ptr())
    return fu, loss


def poisson_adjoint_adam_volumes(fu, h2, scale, out, x, m, v, alphas, one_minus_b1, one_minus_b2, eps):
    """`poisson_adjoint_adam` for the B 3-D members of [B, *shape] arrays in ONE launch.  alphas: DEVICE step sizes, [B]
    (one per member) or one element (shared); out = None: the gradient is not stored."""
    nb, shape = int(fu.shape[0]), tuple(fu.shape[1:])
    assert alphas.dtype == fu.dtype and alphas.is_cuda and alphas.numel() in (1, nb) and alphas.is_contiguous()
    (fp, fs), (xp, xs), (mp, ms), (vp, vs) = (_members(t, nb, shape) for t in (fu, x, m, v))
    gp, gs = _members(out, nb, shape) if out is not None else (None, fs)
    h2a, h2p = host_reals(h2, fu.dtype)
    call("poisson_adjoint_adam_volumes", fu.dtype, fp, gp, xp, mp, vp, c_int(nb), fs, gs, xs, ms, vs, i64(shape),
         c_int(len(shape)), h2p, float(scale), float(one_minus_b1), float(one_minus_b2), float(eps), ptr(alphas),
         c_int64(1 if alphas.numel() == nb and nb > 1 else 0), stream_ptr())
    return out


def mg_synth_adj_adam_members(gu, shapes, loc, grads, x=None, m=None, v=None, alphas=None, one_minus_b1=0.0, one_minus_b2=0.0,
                              eps=0.0, period=0):
    """`mg_synth_adj_adam` on contiguous [R, *shape] level arrays of R rows (`shapes`: the level shapes of ONE row, `loc`:
    its location string, any mix of 'c' and 'n', 1-D to 4-D): one launch per level for all rows, the update of the levels
    >= 1 inside it.  alphas: DEVICE step sizes; row r reads alphas[r % period] (period 0: alphas[r]; one element: shared by
    all rows).  x, m, v all None: the gradients alone.  Entry 0 of grads, x, m, v is not touched (the chain reads gu).
    Per row: the gradients of `mg_synth_adj`, the x, m, v of `adam_step`, bit for bit."""
    nr, nlvl = int(gu.shape[0]), len(shapes)
    assert tuple(gu.shape) == (nr,) + tuple(shapes[0]) and gu.is_contiguous() and len(loc) == len(shapes[0])
    update = x is not None or m is not None or v is not None
    for arrs in (grads,) + ((x, m, v) if update else ()):  # (the launcher takes contiguous [R, *shape] level arrays)
        assert all(tuple(t.shape) == (nr,) + tuple(s) and t.is_contiguous() and t.dtype == gu.dtype
                   for t, s in zip(arrs[1:], shapes[1:]))
    none0 = lambda arrs: ptr_array([None] + list(arrs[1:]))
    stride, period = 0, int(period)
    if update:
        assert alphas.dtype == gu.dtype and alphas.is_cuda and alphas.is_contiguous()
        assert alphas.numel() in (1, period or nr), (alphas.numel(), period, nr)
        stride = 1 if alphas.numel() > 1 else 0
    flat = [int(n) for s in shapes for n in s]
    call("mg_synth_adj_adam_members", gu.dtype, ptr(gu), none0(grads), i64(flat), c_int(nlvl), c_int(len(shapes[0])),
         loc.encode(), c_int(nr), *((none0(x), none0(m), none0(v)) if update else (None, None, None)), float(one_minus_b1),
         float(one_minus_b2), float(eps), ptr(alphas) if update else None, c_int64(stride), c_int64(period), stream_ptr())
    return grads


def mg_synth_members(terms, loc, work=None, out=None):
    """`mg_synth` (factors 1) on contiguous [R, *shape] level arrays of R rows (`loc`: the location string of ONE row, any
    mix of 'c' and 'n', 1-D to 4-D): one launch per level for all rows, row r the bits of `mg_synth` on that row alone.
    Rows of four axes, which have no '.' + loc view, run the fast prolongation where it takes the layout and the generic
    one elsewhere, the row on a grid dimension."""
    nlvl, nr = len(terms), int(terms[0].shape[0])
    shapes = [tuple(int(n) for n in t.shape[1:]) for t in terms]
    assert len(loc) == len(shapes[0]) and all(t.shape[0] == nr and t.is_contiguous() and t.dtype == terms[0].dtype for t in terms)
    if out is None:
        out = torch.empty_like(terms[0])
    if work is None:
        work = ([None] + [torch.empty_like(t) for t in terms[1:-1]] + [None])[:nlvl]
    assert out.shape == terms[0].shape and out.is_contiguous() and out.dtype == terms[0].dtype
    assert all(w is None or (w.shape == t.shape and w.is_contiguous() and w.dtype == t.dtype) for w, t in zip(work, terms))
    call("mg_synth_members", terms[0].dtype, ptr_array(terms), ptr_array(work), ptr(out), i64([n for s in shapes for n in s]),
         c_int(nlvl), c_int(len(shapes[0])), loc.encode(), c_int(nr), stream_ptr())
    return out


def jacobi2_supported(shape, dtype):
    """Arrays whose rows are whole 16-byte packs (odil_poisson_jacobi2, odil_stencil_var_smooth2)."""
    pack = 2 if dtype == torch.float64 else 4
    return 1 <= len(shape) <= 3 and shape[-1] % pack == 0 and min(shape) >= 2


def poisson_jacobi2(u, rhs, h2, omega1, omega2, out, zc_hint=0):
    """Two damped-Jacobi sweeps (weights omega1, then omega2) in ONE pass: bit-identical to two calls of
    `poisson_jacobi`, 3 words per cell instead of 6 (out is not u).  u = None: from the zero vector (2 words)."""
    assert rhs.shape == out.shape and jacobi2_supported(tuple(rhs.shape), rhs.dtype)
    assert u is None or (u.shape == rhs.shape and out.data_ptr() != u.data_ptr() and u.is_contiguous())
    assert rhs.is_contiguous() and out.is_contiguous()
    h2a, h2p = host_reals(h2, rhs.dtype)
    call("poisson_jacobi2", rhs.dtype, ptr(u) if u is not None else None, ptr(rhs), ptr(out), i64(rhs.shape),
         c_int(rhs.dim()), h2p, float(omega1), float(omega2), c_int(zc_hint), stream_ptr())
    return out


def poisson_jacobi2_synth(coarse, x, rhs, h2, omega1, omega2, out, zc_hint=0):
    """Two sweeps (weights omega1, omega2) of u = x + P coarse in ONE pass: the coarse-grid correction of a V-cycle and
    its post-smoothing; bit-identical to `interp_add` + `poisson_jacobi2` (out is not x; see jacobi_synth_supported)."""
    assert coarse.dim() == 3 and tuple(x.shape) == tuple(2 * s for s in coarse.shape) and x.shape == rhs.shape == out.shape
    assert coarse.is_contiguous() and x.is_contiguous() and rhs.is_contiguous() and out.data_ptr() != x.data_ptr()
    h2a, h2p = host_reals(h2, x.dtype)
    call("poisson_jacobi2_synth", x.dtype, ptr(coarse), ptr(x), ptr(rhs), ptr(out), i64(coarse.shape), h2p, float(omega1),
         float(omega2), c_int(zc_hint), stream_ptr())
    return out


def jacobi_synth_supported(shape, dtype):
    """3-D arrays with even extents >= 4 (the coarse array they are prolongated from has extents >= 2)."""
    return len(shape) == 3 and all(s % 2 == 0 and s >= 4 for s in shape)


def poisson_jacobi_synth(coarse, x, rhs, h2, omega, out):
    """out = u - omega (A u - rhs) / diag(A) with u = x + P coarse formed in registers: the coarse-grid correction of
    a V-cycle and its first post-smoothing sweep in one pass (out is not x)."""
    assert coarse.dim() == 3 and tuple(x.shape) == tuple(2 * s for s in coarse.shape) and x.shape == rhs.shape == out.shape
    assert coarse.is_contiguous() and x.is_contiguous() and rhs.is_contiguous() and out.data_ptr() != x.data_ptr()
    h2a, h2p = host_reals(h2, x.dtype)
    call("poisson_jacobi_synth", x.dtype, ptr(coarse), ptr(x), ptr(rhs), ptr(out), i64(coarse.shape), h2p, float(omega),
         stream_ptr())
    return out


def poisson_residual_synth(coarse, w0, rhs, h2, fu=None, loss=None, zrange=None, denom=None):
    """fu = Lap(w0 + P coarse) - rhs, loss = mean(fu**2): the residual with the last prolongation of
    the multigrid synthesis fused in (u is never stored).  3-D cell-centred arrays, w0.shape == 2 * coarse.shape.
    zrange=(z0, z1) / denom: slab variant, loss = sum over fine planes z0 <= z < z1 of fu^2 / denom."""
    from ctypes import c_double

    assert coarse.dim() == 3 and tuple(w0.shape) == tuple(2 * s for s in coarse.shape) and w0.shape == rhs.shape
    assert coarse.is_contiguous() and w0.is_contiguous() and rhs.is_contiguous()
    if fu is None:
        fu = torch.empty_like(w0)
    if loss is None:
        loss = torch.empty((), dtype=w0.dtype, device=w0.device)
    h2a, h2p = host_reals(h2, w0.dtype)
    sums = residual_synth_workspace(w0.device, coarse.shape)
    call(
        "poisson_residual_synth", w0.dtype, ptr(coarse), ptr(w0), ptr(rhs), ptr(fu), i64(coarse.shape), h2p,
        c_int64(zrange[0] if zrange else 0), c_int64(zrange[1] if zrange else -1), c_double(float(denom or 0.0)),
        ptr(reduce_workspace(w0.device)), ptr(sums), c_size_t(sums.numel() * 8), ptr(loss), stream_ptr(),
    )
    return fu, loss


def poisson_adjoint(fu, h2, scale, out=None):
    """gu = J^T (scale * fu)."""
    if out is None:
        out = torch.empty_like(fu)
    h2a, h2p = host_reals(h2, fu.dtype)
    call("poisson_adjoint", fu.dtype, ptr(fu), ptr(out), i64(fu.shape), c_int(fu.dim()), h2p, float(scale), stream_ptr())
    return out


def poisson_adjoint_adam(fu, h2, scale, out, x, m, v, alpha, one_minus_b1, one_minus_b2, eps):
    """gu = J^T (scale * fu) written to `out`, and the Adam step of (x, m, v) with that gradient,
    in the same launch (x, m, v: arrays of fu's shape, updated in place)."""
    assert x.shape == fu.shape and m.numel() == v.numel() == fu.numel()
    h2a, h2p = host_reals(h2, fu.dtype)
    a, adev = _step_size(alpha, fu.dtype)
    call(
        # (out=None: the gradient is consumed by the update, not stored)
        "poisson_adjoint_adam", fu.dtype, ptr(fu), ptr(out), ptr(x), ptr(m), ptr(v), i64(fu.shape), c_int(fu.dim()),
        h2p, float(scale), a, float(one_minus_b1), float(one_minus_b2), float(eps), adev, stream_ptr(),
    )
    return out


def adjoint_transpose_supported(shape):
    """Sizes at which the one-pass stencil adjoint + first transposed prolongation pays (and is defined)."""
    return len(shape) == 3 and all(n % 2 == 0 for n in shape) and shape[0] >= 8 and shape[1] >= 32 and shape[2] >= 128


def poisson_adjoint_transpose(fu, h2, scale, g1, g0=None, adam0=None, adam1=None, alpha=0.0, one_minus_b1=0.0,
                              one_minus_b2=0.0, eps=0.0, cut=(False, False), plan=None):
    """g0 = J^T (scale * fu) (stored only if `g0` is given), g1 = P^T g0, and the Adam steps of the finest level
    (adam0 = (x, m, v)) and of the next one (adam1) inside the same launch: g0 never goes through memory.
    cut=(lo, hi): that end of axis 0 is a slab interface (ghost planes), not a wall.
    plan=(L, Zs, S): the cut of the coarse z axis into units of work (include/odil_hip.h:
    odil_poisson_adjoint_transpose_adam_plan; the same bits for every plan); None: the library's rule."""
    assert fu.dim() == 3 and tuple(g1.shape) == tuple(n // 2 for n in fu.shape) and fu.is_contiguous()
    h2a, h2p = host_reals(h2, fu.dtype)
    a, adev = _step_size(alpha, fu.dtype)
    a0 = adam0 if adam0 is not None else (None, None, None)
    a1 = adam1 if adam1 is not None else (None, None, None)
    for t in list(a0) + list(a1):
        assert t is None or (t.is_contiguous() and t.dtype == fu.dtype)
    if plan is not None:
        L, Zs, S = (int(p) for p in plan)
        if not 1 <= S <= L <= 64 or not 0 <= Zs <= g1.shape[0]:
            raise ValueError("plan (L, Zs, S) = {} needs 1 <= S <= L <= 64 and 0 <= Zs <= {}".format(plan, g1.shape[0]))
        call(
            "poisson_adjoint_transpose_adam_plan", fu.dtype, ptr(fu), ptr(g0), ptr(g1), i64(fu.shape), h2p, float(scale),
            ptr(a0[0]), ptr(a0[1]), ptr(a0[2]), ptr(a1[0]), ptr(a1[1]), ptr(a1[2]), a, float(one_minus_b1),
            float(one_minus_b2), float(eps), adev, c_int(1 if cut[0] else 0), c_int(1 if cut[1] else 0), c_int(L),
            c_int(Zs), c_int(S), stream_ptr(),
        )
        return g1
    call(
        "poisson_adjoint_transpose_adam", fu.dtype, ptr(fu), ptr(g0), ptr(g1), i64(fu.shape), h2p, float(scale),
        ptr(a0[0]), ptr(a0[1]), ptr(a0[2]), ptr(a1[0]), ptr(a1[1]), ptr(a1[2]), a, float(one_minus_b1),
        float(one_minus_b2), float(eps), adev, c_int(1 if cut[0] else 0), c_int(1 if cut[1] else 0), stream_ptr(),
    )
    return g1


def adjoint_transpose_plan(shape, transpose_only=False):
    """(L, Zs, S) that poisson_adjoint_transpose takes by itself on a fine array of `shape` (Zs == shape[0] // 2: one
    tier of chunks of L planes); transpose_only: that of interp_adj(..., "ccc") on float64 where its LDS-tile kernel runs."""
    out = (c_int * 3)()
    if _lib.load().odil_tile_sched_rule(i64(shape), 1 if transpose_only else 0, out) != 0:
        raise ValueError("adjoint_transpose_plan: shape {}".format(tuple(shape)))
    return tuple(out)


def tile_sched_units(Z, Y, XS, L, Zs, S):
    """[(z0, z1, y, xs) or None per workgroup] of the two-tier schedule of the tile transposes, by the kernels' own decode
    run on the host (include/odil_hip.h: odil_tile_sched_units)."""
    lib = _lib.load()
    grid = lib.odil_tile_sched_units(Z, Y, XS, L, Zs, S, None, 0)
    if grid < 0:
        raise ValueError("tile_sched_units: ({}, {}, {}) is not a plan for {} planes".format(L, Zs, S, Z))
    buf = (c_int32 * (4 * grid))()
    lib.odil_tile_sched_units(Z, Y, XS, L, Zs, S, buf, grid)
    flat = list(buf)
    return [None if flat[4 * b] < 0 else tuple(flat[4 * b:4 * b + 4]) for b in range(grid)]


def poisson_jac_match(arrays, shape, h2):
    """[(2 d + 1), 2] device tensor: per coefficient array (centre, -e_0, +e_0, ...) max |a_k - e_k| and max |e_k| against the
    Poisson Jacobian's values, formed on the fly in ONE pass (include/odil_hip.h: odil_poisson_jac_match)."""
    from ._lib import ptr_array

    ndim = len(shape)
    assert len(arrays) == 2 * ndim + 1 and all(a.numel() == math.prod(shape) for a in arrays)
    arrays = [a.reshape(-1) if a.is_contiguous() else a.reshape(-1).contiguous() for a in arrays]
    dtype = arrays[0].dtype
    h2a, h2p = host_reals(h2, dtype)
    out = torch.empty((2 * ndim + 1, 2), dtype=dtype, device=arrays[0].device)
    call("poisson_jac_match", dtype, ptr_array(arrays), i64(shape), c_int(ndim), h2p, ptr(reduce_workspace(out.device)), ptr(out),
         stream_ptr())
    return out


def poisson_jac_coeffs(shape, h2, dtype, device):
    """(2*ndim+1, *shape) coefficient arrays [centre, -1 ax0, +1 ax0, ...] (reference core.py:1313-1361)."""
    ndim = len(shape)
    out = torch.empty((2 * ndim + 1,) + tuple(shape), dtype=dtype, device=device)
    h2a, h2p = host_reals(h2, dtype)
    call("poisson_jac_coeffs", dtype, ptr(out), i64(shape), c_int(ndim), h2p, stream_ptr())
    return out


_dense_ws = {}
_dense_wide_ws = {}
DENSE_NARROW_COLUMNS = 64  # per operand: odil_dense_block_xty
DENSE_WIDE_COLUMNS = 1024  # per operand: odil_dense_block_xty_wide


def dense_xty(x, y):
    """X^T Y of two tall, skinny matrices (rows x <= 1024 columns each, row-major, any row stride) on the matrix
    cores: v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, deterministic two-stage reduction.  The dense block of
    the Newton normal equations (reference core.py:1189-1203, linsolver.py:17-23).  Up to 64 columns per operand: one
    workgroup per row range; beyond: 64-column panels (odil_dense_block_xty_wide).  There, when x and y are views of
    the SAME memory with the same row stride and x has no more columns than y (D^T D, D^T [D | r]), the panel pairs
    below the diagonal are mirrored from those above it: out[:, :px] is symmetric to the bit, and differs in the last
    bits from what a contiguous copy of x against y gives (that call computes every pair)."""
    assert x.dim() == 2 and y.dim() == 2 and x.shape[0] == y.shape[0] and x.dtype == y.dtype
    assert x.stride(1) == 1 and y.stride(1) == 1
    px, py = x.shape[1], y.shape[1]
    if max(px, py) > DENSE_WIDE_COLUMNS:
        raise ValueError("dense_xty: {} x {} columns; at most {} per operand".format(px, py, DENSE_WIDE_COLUMNS))
    key = (str(x.device), x.dtype)
    out = torch.empty((px, py), dtype=x.dtype, device=x.device)
    if max(px, py) <= DENSE_NARROW_COLUMNS:
        ws = _dense_ws.get(key)
        if ws is None:
            ws = _dense_ws[key] = torch.empty(_lib.load().odil_dense_block_workspace_bytes() // 8, dtype=torch.float64,
                                              device=x.device).view(x.dtype)
        call("dense_block_xty", x.dtype, c_void_p(x.data_ptr()), c_void_p(y.data_ptr()), c_int64(x.shape[0]),
             c_int(px), c_int(py), c_int64(x.stride(0)), c_int64(y.stride(0)), ptr(out), ptr(ws), stream_ptr())
        return out
    need = _lib.load().odil_dense_block_wide_workspace_bytes(px, py)
    ws = _dense_wide_ws.get(key)
    if ws is None or ws.numel() * ws.element_size() < need:  # grown on demand, never beyond the kernel's 64 MiB
        ws = _dense_wide_ws[key] = torch.empty(need // 8, dtype=torch.float64, device=x.device).view(x.dtype)
    call("dense_block_xty_wide", x.dtype, c_void_p(x.data_ptr()), c_void_p(y.data_ptr()), c_int64(x.shape[0]),
         c_int(px), c_int(py), c_int64(x.stride(0)), c_int64(y.stride(0)), ptr(out), ptr(ws),
         c_size_t(ws.numel() * ws.element_size()), stream_ptr())
    return out


def adam_step(x, m, v, g, alpha, one_minus_b1, one_minus_b2, eps):
    """In-place AdamNativeOptimizer._step on flat vectors (reference optimizer.py:311-319)."""
    assert x.numel() == m.numel() == v.numel() == g.numel()
    a, adev = _step_size(alpha, x.dtype)
    call(
        "adam_step", x.dtype, ptr(x), ptr(m), ptr(v), ptr(g), c_int64(x.numel()), a, float(one_minus_b1),
        float(one_minus_b2), float(eps), adev, stream_ptr(),
    )


def adam_step_batch(x, m, v, g, alphas, one_minus_b1, one_minus_b2, eps):
    """`adam_step` for the B members of [B, *shape] arrays in ONE launch (the members contiguous, possibly padded: the
    leading strides are the member strides, as `_members` describes them).  alphas: DEVICE step sizes, [B] (one per
    member) or one element (shared).  Member b gets the bits of `adam_step` on its own arrays."""
    nb, shape = int(x.shape[0]), tuple(x.shape[1:])
    assert x.dtype == m.dtype == v.dtype == g.dtype == alphas.dtype
    assert alphas.is_cuda and alphas.numel() in (1, nb) and alphas.is_contiguous()
    (xp, xs), (mp, ms), (vp, vs), (gp, gs) = (_members(t, nb, shape) for t in (x, m, v, g))
    call("adam_step_batch", x.dtype, xp, mp, vp, gp, c_int(nb), c_int64(x[0].numel()), xs, ms, vs, gs, float(one_minus_b1),
         float(one_minus_b2), float(eps), ptr(alphas), c_int64(1 if alphas.numel() == nb and nb > 1 else 0), stream_ptr())


def param_rows(rows, npg, device):
    """The index map of `adam_step_params_batch` as a DEVICE int32 tensor, checked on the host: rows [P], or [B, P] (a map
    per member), every entry -1 (no grid gradient for that packed parameter) or a row 0 ... npg - 1 of `pgrad`."""
    rows = torch.tensor(rows, dtype=torch.int64)
    if rows.dim() not in (1, 2) or (rows.numel() and (int(rows.min()) < -1 or int(rows.max()) >= int(npg))):
        raise ValueError("param_rows: entries are -1 or rows 0 ... {} of the parameter gradients".format(int(npg) - 1))
    return rows.to(torch.int32).contiguous().to(device)


def adam_step_params_batch(x, m, v, g, pgrad, rows, alphas=None, one_minus_b1=0.0, one_minus_b2=0.0, eps=0.0, extra=None):
    """The Array unknowns of the B members of an ensemble in ONE launch: g[b, p] = pgrad[b, rows[p]] (0 where rows[p] is
    -1) and `adam_step` of x, m, v [B, P] with that gradient.  pgrad: [B, npg] (rows contiguous, any row stride >= npg);
    rows: `param_rows` ([P], or [B, P]); alphas: DEVICE step sizes, [B] or one element (shared).  x, m, v all None: only
    g is formed.  Member b gets the bits of `adam_step` on its own arrays.
    extra [B, P] (odil_adam_step_params_extra_batch): the part of the gradient a generated `k_par_batch` left, added to
    the rows' before the update and cleared by the launch."""
    nb, npar = int(g.shape[0]), int(g.shape[1])
    assert g.dim() == 2 and g.is_contiguous() and g.dtype == pgrad.dtype
    assert pgrad.dim() == 2 and pgrad.shape[0] == nb and (pgrad.shape[1] == 0 or pgrad.stride(1) == 1) and pgrad.is_cuda
    assert rows.dtype == torch.int32 and rows.is_cuda and rows.is_contiguous()
    assert tuple(rows.shape) in ((npar,), (nb, npar)), (tuple(rows.shape), (nb, npar))
    update = x is not None or m is not None or v is not None
    if update:
        assert all(t is not None and t.shape == g.shape and t.dtype == g.dtype and t.is_contiguous() for t in (x, m, v))
        assert alphas.dtype == g.dtype and alphas.is_cuda and alphas.numel() in (1, nb) and alphas.is_contiguous()
    pstride = max(int(pgrad.stride(0)), int(pgrad.shape[1])) if nb > 1 else int(pgrad.shape[1])
    more = ()
    if extra is not None:
        assert extra.shape == g.shape and extra.dtype == g.dtype and extra.is_contiguous() and extra.is_cuda
        more = (ptr(extra),)
    call("adam_step_params_extra_batch" if more else "adam_step_params_batch", g.dtype, ptr(x), ptr(m), ptr(v), ptr(g),
         c_void_p(pgrad.data_ptr()), *more, ptr(rows), c_int(nb), c_int64(npar), c_int(int(pgrad.shape[1])), c_int64(pstride), c_int64(npar if rows.dim() == 2 else 0),
         float(one_minus_b1), float(one_minus_b2), float(eps), ptr(alphas) if update else None,
         c_int64(1 if update and alphas.numel() == nb and nb > 1 else 0), stream_ptr())


def adam_step_pieces(x, m, v, g, npieces, stride, offset, count, alpha, one_minus_b1, one_minus_b2, eps):
    """adam_step on the elements o * stride + offset + j (o < npieces, j < count) of four flat vectors."""
    assert x.numel() == m.numel() == v.numel() == g.numel() and x.is_contiguous()
    assert npieces == 0 or (npieces - 1) * stride + offset + count <= x.numel()
    a, adev = _step_size(alpha, x.dtype)
    call(
        "adam_step_pieces", x.dtype, ptr(x), ptr(m), ptr(v), ptr(g), c_int64(npieces), c_int64(stride), c_int64(offset),
        c_int64(count), a, float(one_minus_b1), float(one_minus_b2), float(eps), adev, stream_ptr(),
    )


def axpy(y, x, a):
    """y += a * x in place."""
    assert y.numel() == x.numel() and y.dtype == x.dtype
    call("axpy", y.dtype, ptr(y), ptr(x), c_int64(y.numel()), float(a), stream_ptr())
    return y


def scale(x, a, adev=None, out=None):
    """out = a * (adev[0] if adev is given) * x."""
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    call("scale", x.dtype, ptr(x), ptr(out), c_int64(x.numel()), float(a), ptr(adev), stream_ptr())
    return out


def addcmul(y, a, b, accumulate=True):
    """y (+)= a * b elementwise, in place."""
    assert y.numel() == a.numel() == b.numel()
    call("addcmul", y.dtype, ptr(y), ptr(a), ptr(b), c_int64(y.numel()), c_int(1 if accumulate else 0), stream_ptr())
    return y


_dots_ws = {}


def dots_workspace(device, nvec):
    key = str(device)
    ws = _dots_ws.get(key)
    need = _lib.load().odil_dots_workspace_bytes(nvec) // 8
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float64, device=device)
        _dots_ws[key] = ws
    return ws


def dots(a, b, out=None):
    """out[k] = <a[k], b> for a of shape (nvec, n); deterministic, f64 accumulation."""
    if a.dim() == 1:
        a = a[None]
    nvec, n = a.shape
    assert b.numel() == n and a.stride(1) == 1
    if out is None:
        out = torch.empty(nvec, dtype=a.dtype, device=a.device)
    call(
        "dots", a.dtype, ptr_strided(a), c_int64(a.stride(0)), c_int(nvec), ptr(b), c_int64(n),
        ptr(dots_workspace(a.device, nvec)), ptr(out), stream_ptr(),
    )
    return out


def dots3(a, bs, out=None):
    """out[j, k] = <a[k], bs[j]> for up to three vectors bs, reading a once."""
    if a.dim() == 1:
        a = a[None]
    nvec, n = a.shape
    bs = list(bs) + [None] * (3 - len(bs))
    assert a.stride(1) == 1 and all(b is None or b.numel() == n for b in bs)
    if out is None:
        out = torch.empty((3, nvec), dtype=a.dtype, device=a.device)
    call(
        "dots3", a.dtype, ptr_strided(a), c_int64(a.stride(0)), c_int(nvec), ptr(bs[0]), ptr(bs[1]), ptr(bs[2]),
        c_int64(n), ptr(dots_workspace(a.device, 3 * nvec)), ptr(out), stream_ptr(),
    )
    return out


def lbfgs_probe(g, d, out):
    """out[:3] = (<g, d>, <g, g>, max |g|) in one pass over g."""
    assert g.numel() == d.numel() and g.dtype == d.dtype == out.dtype and out.numel() >= 3
    call("lbfgs_probe", g.dtype, ptr(g), ptr(d), c_int64(g.numel()), ptr(dots_workspace(g.device, 3)), ptr(out),
         stream_ptr())
    return out


def ptr_strided(a):
    import ctypes

    if not a.is_cuda:
        raise _lib.OdilHipError("tensor is on '{}': the HIP kernels need device memory".format(a.device))
    return ctypes.c_void_p(a.data_ptr())


def lincomb(y, beta, a, coef):
    """y = beta*y + sum_k coef[k] * a[k]  (coef: device tensor)."""
    if a.dim() == 1:
        a = a[None]
    nvec, n = a.shape
    assert y.numel() == n and coef.numel() == nvec and (a.stride(1) == 1 or n == 1), (tuple(y.shape), tuple(a.shape), a.stride())
    call(
        "lincomb", y.dtype, ptr(y), float(beta), ptr_strided(a), c_int64(a.stride(0)), c_int(nvec), ptr(coef),
        c_int64(n), stream_ptr(),
    )
    return y


# ---- the L-BFGS algebra of an ensemble in lock-step (odil_lbfgs_*_batch): member-major [B, n] vectors whose rows are
# contiguous (the leading stride is the member stride: members may be padded), a [B, rows, n] history, a list of members
# per launch (`members`: DEVICE int32 tensor, None = all), scalars and counts of a member in entry b of DEVICE arrays.
def _rows(t, nb, n):
    """(device pointer, member stride in elements) of a [B, n] tensor with contiguous rows."""
    assert t.dim() == 2 and tuple(t.shape) == (nb, n) and (t.stride(1) == 1 or n == 1), (tuple(t.shape), t.stride())
    if not t.is_cuda:
        raise _lib.OdilHipError("tensor is on '{}': the HIP kernels need device memory (no CPU fallback)".format(t.device))
    return c_void_p(t.data_ptr()), c_int64(t.stride(0) if nb > 1 else max(t.stride(0), n))


def _history(w, nb, n):
    """(device pointer, member stride, lda, rows) of a [B, rows, n] history."""
    assert w.dim() == 3 and w.shape[0] == nb and w.shape[2] == n and (w.stride(2) == 1 or n == 1), (tuple(w.shape), w.stride())
    if not w.is_cuda:
        raise _lib.OdilHipError("tensor is on '{}': the HIP kernels need device memory (no CPU fallback)".format(w.device))
    rows = int(w.shape[1])
    lda = w.stride(1) if rows > 1 else max(w.stride(1), n)
    return c_void_p(w.data_ptr()), c_int64(w.stride(0) if nb > 1 else max(w.stride(0), (rows - 1) * lda + n)), c_int64(lda), rows


def _member_list(members, nb):
    if members is None:
        return None, c_int(nb)
    assert members.dtype == torch.int32 and members.is_cuda and members.is_contiguous() and members.dim() == 1
    return c_void_p(members.data_ptr()), c_int(members.numel())


def _per_member(t, nb, dtype):
    if t is None:
        return None
    assert t.dtype == dtype and t.is_cuda and t.is_contiguous() and t.numel() == nb, (t.dtype, tuple(t.shape))
    return c_void_p(t.data_ptr())


def lbfgs_batch_partials(n, max_count, dtype):
    """Doubles of reduction workspace ONE member of `lbfgs_probe_batch` / `lbfgs_dots3_batch` needs."""
    return int(_lib.load().odil_lbfgs_batch_partials(c_int64(n), c_int(max_count), 8 if dtype == torch.float64 else 4))


def _partials_args(partials, nb):
    assert partials.dtype == torch.float64 and partials.dim() == 2 and partials.shape[0] == nb and partials.stride(1) == 1
    if not partials.is_cuda:
        raise _lib.OdilHipError("the partials workspace is on '{}': the HIP kernels need device memory".format(partials.device))
    stride = max(partials.stride(0), partials.shape[1])
    return c_void_p(partials.data_ptr()), c_int64(stride), c_int64((nb - 1) * stride + partials.shape[1])


def lbfgs_probe_batch(g, d, out, partials, members=None):
    """out[b, :3] = `lbfgs_probe(g[b], d[b])` for the listed members of [B, n] vectors, bit for bit: one launch + one
    reduction launch.  out: [B, >= 3] with contiguous rows; partials: [B, >= lbfgs_batch_partials(n, 1)] float64."""
    nb, n = int(g.shape[0]), int(g.shape[1])
    assert g.dtype == d.dtype == out.dtype and out.dim() == 2 and out.shape[0] == nb and out.shape[1] >= 3 and out.stride(1) == 1
    (gp, gs), (dp, ds) = _rows(g, nb, n), _rows(d, nb, n)
    mp, nsel = _member_list(members, nb)
    call("lbfgs_probe_batch", g.dtype, gp, gs, dp, ds, c_int64(n), c_int(nb), mp, nsel, *_partials_args(partials, nb),
         c_void_p(out.data_ptr()), c_int64(out.stride(0) if nb > 1 else max(out.stride(0), 3)), stream_ptr())
    return out


def lbfgs_dots3_batch(w, counts, max_count, bs, out, partials, members=None):
    """out[b, j, k] = <w[b, k], bs[j][b]> for k < counts[b] (counts: DEVICE int32 [B], None: max_count for all) and up to
    three [B, n] vectors bs: `dots3(w[b, :counts[b]], [bs[j][b]])` for the listed members, bit for bit.  out: [B, 3, ldo]
    with ldo >= max_count; entries k >= counts[b] are left alone.  w: [B, rows, n], or [B, n] (one vector per member)."""
    if w.dim() == 2:
        w = w[:, None, :]
    nb, n = int(w.shape[0]), int(w.shape[2])
    wp, ws, lda, rows = _history(w, nb, n)
    if rows == 1:
        lda = c_int64(n)  # (what `dots3(d[None], ...)` of one member passes)
    bs = list(bs) + [None] * (3 - len(bs))
    b = [_rows(t, nb, n) if t is not None else (None, c_int64(0)) for t in bs]
    assert out.dtype == w.dtype and out.dim() == 3 and out.shape[0] == nb and out.shape[1] == 3 and out.stride(2) == 1
    assert out.shape[2] >= max_count and (out.stride(1) >= out.shape[2] or out.shape[2] == 1)
    mp, nsel = _member_list(members, nb)
    ldo = out.stride(1)
    call("lbfgs_dots3_batch", w.dtype, wp, ws, lda, c_int(rows), _per_member(counts, nb, torch.int32), c_int(max_count),
         b[0][0], b[0][1], b[1][0], b[1][1], b[2][0], b[2][1], c_int64(n), c_int(nb), mp, nsel,
         *_partials_args(partials, nb), c_void_p(out.data_ptr()),
         c_int64(out.stride(0) if nb > 1 else max(out.stride(0), 2 * ldo + max_count)), c_int64(ldo), stream_ptr())
    return out


def lbfgs_lincomb_batch(y, beta, w, counts, max_count, coef, members=None):
    """y[b] = beta y[b] + sum_{k < counts[b]} coef[b, k] w[b, k] for the listed members: `lincomb` per member, bit for bit."""
    nb, n = int(y.shape[0]), int(y.shape[1])
    wp, ws, lda, rows = _history(w, nb, n)
    (yp, ys), (cp, cs) = _rows(y, nb, n), _rows(coef, nb, int(coef.shape[1]))
    assert coef.dtype == y.dtype == w.dtype and coef.shape[1] >= max_count
    mp, nsel = _member_list(members, nb)
    call("lbfgs_lincomb_batch", y.dtype, yp, ys, float(beta), wp, ws, lda, c_int(rows), _per_member(counts, nb, torch.int32),
         c_int(max_count), cp, cs, c_int64(n), c_int(nb), mp, nsel, stream_ptr())
    return y


def lbfgs_axpy_batch(out, y, x, alpha, members=None):
    """out[b] = y[b] + alpha[b] x[b] (`axpy`; out may be y) for the listed members; y = None: out[b] = alpha[b] x[b]
    (`scale`); y = alpha = None: out[b] = x[b].  alpha: DEVICE [B]."""
    nb, n = int(x.shape[0]), int(x.shape[1])
    assert out.dtype == x.dtype and (y is None or y.dtype == x.dtype)
    (op, os_), (xp, xs) = _rows(out, nb, n), _rows(x, nb, n)
    yp, ys = _rows(y, nb, n) if y is not None else (None, c_int64(0))
    mp, nsel = _member_list(members, nb)
    call("lbfgs_axpy_batch", x.dtype, op, os_, yp, ys, xp, xs, _per_member(alpha, nb, x.dtype), c_int64(n), c_int(nb), mp,
         nsel, stream_ptr())
    return out


def lbfgs_pair_batch(g, r, d, w, stp, slot, members=None):
    """The correction pair of the listed members in one launch: r[b] = g[b] - r[b], d[b] = stp[b] d[b] and, where
    slot[b] >= 0, w[b, 2 slot[b]] = d[b], w[b, 2 slot[b] + 1] = r[b].  stp: DEVICE [B]; slot: DEVICE int32 [B]."""
    nb, n = int(g.shape[0]), int(g.shape[1])
    assert g.dtype == r.dtype == d.dtype == w.dtype
    wp, ws, lda, rows = _history(w, nb, n)
    (gp, gs), (rp, rs), (dp, ds) = _rows(g, nb, n), _rows(r, nb, n), _rows(d, nb, n)
    mp, nsel = _member_list(members, nb)
    call("lbfgs_pair_batch", g.dtype, gp, gs, rp, rs, dp, ds, wp, ws, lda, c_int(rows), _per_member(stp, nb, g.dtype),
         _per_member(slot, nb, torch.int32), c_int64(n), c_int(nb), mp, nsel, stream_ptr())


def poisson_adjoint_batch(fu, h2, scale, out):
    """out[b] = `poisson_adjoint(fu[b])` for the B members of [B, *shape] arrays (1-D to 3-D) in ONE launch, no update."""
    nb, shape = int(fu.shape[0]), tuple(fu.shape[1:])
    (fp, fs), (gp, gs) = _members(fu, nb, shape), _members(out, nb, shape)
    h2a, h2p = host_reals(h2, fu.dtype)
    call("poisson_adjoint_batch", fu.dtype, fp, gp, c_int(nb), fs, gs, i64(shape), c_int(len(shape)), h2p, float(scale),
         stream_ptr())
    return out


def stencil_apply(coeffs, shifts, x, transpose=False, out=None):
    """y = M x or M^T x for the stencil matrix with per-shift coefficient arrays
    (reference core.py:1144-1171)."""
    nshift = len(shifts)
    ndim = x.dim()
    if out is None:
        out = torch.empty_like(x)
    flat = []
    for s in shifts:
        flat += list(s)
    call(
        "stencil_apply", x.dtype, ptr(coeffs), i64(flat), c_int(nshift), ptr(x), ptr(out), i64(x.shape), c_int(ndim),
        c_int(1 if transpose else 0), stream_ptr(),
    )
    return out


def stencil_march(coeffs, shifts, diag, b, axis, direction, out=None):
    """x with M x = b for a stencil matrix triangular along `axis` (see odil_stencil_march in the header)."""
    if out is None:
        out = torch.empty_like(b)
    flat = []
    for s in shifts:
        flat += list(s)
    call("stencil_march", b.dtype, ptr(coeffs), i64(flat), c_int(len(shifts)), c_int(diag), ptr(b), ptr(out),
         i64(b.shape), c_int(b.dim()), c_int(axis), c_int(direction), stream_ptr())
    return out


class PlaneList:
    """Planes of arrays inside one packed vector and their places in a contiguous message buffer (see
    odil_planes_copy in the header).  planes: [(base, outer, ostride, inner)] in message order; start: where the first
    plane begins in the message (lists over different arrays can share one message); `count`: the message length
    up to the end of this list's planes."""

    def __init__(self, planes, device, start=0):
        rows, off, self.max_count = [], int(start), 1
        for base, outer, ostride, inner in planes:
            rows.append((int(base), int(outer), int(ostride), int(inner), off))
            off += int(outer) * int(inner)
            self.max_count = max(self.max_count, int(outer) * int(inner))
        self.count, self.n = off, len(rows)
        self.vec_ok = int(all(r[3] % 4 == 0 for r in rows))
        self.descs = torch.tensor(rows or [[0] * 5], dtype=torch.int64, device=device).contiguous()

    def _run(self, arr, buf, mode):
        assert buf.numel() >= self.count and buf.dtype == arr.dtype and arr.dim() == 1
        if self.n:
            call("planes_copy", arr.dtype, ptr(arr), ptr(buf), ptr(self.descs), c_int(self.n), c_int64(self.max_count),
                 c_int(self.vec_ok), c_int(mode), stream_ptr())
        return buf

    def pack(self, arr, out=None):
        """The planes of `arr` (flat packed vector) as one contiguous message."""
        if out is None:
            out = torch.empty(self.count, dtype=arr.dtype, device=arr.device)
        return self._run(arr, out, 0)

    def unpack(self, arr, buf):
        self._run(arr, buf, 1)

    def unpack_add(self, arr, buf):
        self._run(arr, buf, 2)


def csr_assemble(coeffs, shifts, shape, col_offset=0):
    """(indptr, indices, data) of the stencil matrix (reference core.py:1144-1171)."""
    nshift = len(shifts)
    size = math.prod(shape)
    dev = coeffs.device
    indptr = torch.empty(size + 1, dtype=torch.int64, device=dev)
    indices = torch.empty(size * nshift, dtype=torch.int64, device=dev)
    data = torch.empty(size * nshift, dtype=coeffs.dtype, device=dev)
    flat = []
    for s in shifts:
        flat += list(s)
    call(
        "csr_assemble", coeffs.dtype, ptr(coeffs), i64(flat), c_int(nshift), i64(shape), c_int(len(shape)),
        c_int64(col_offset), ptr(indptr), ptr(indices), ptr(data), stream_ptr(),
    )
    return indptr, indices, data


# ---- multigrid for the normal equations of several grid fields (csrc/block_mg.hip, gmg.NormalGMG) ------------------
def bmg_apply(coef, table, desc, x, y, b=None, dinv=None, mode=0, omega=0.0):
    """One launch over all fields of a level (include/odil_hip.h: odil_bmg_apply): mode 0 y = A x, 1 y = b - A x,
    2 y = x + omega dinv (b - A x), 3 y = omega dinv b.  desc: the level's host descriptor (c_int64 array)."""
    assert y.is_contiguous() and (x is None or x.data_ptr() != y.data_ptr())
    call("bmg_apply", y.dtype, ptr(coef), ptr(table), desc, ptr(x), ptr(b), ptr(dinv), ptr(y), c_int(mode), float(omega),
         stream_ptr())
    return y


def bmg_assemble(c1, c2, rmap, ashape, rshape, out):
    """out += c1[r(j)] c2[r(j)] over field a's grid (one term of M^T M, odil_bmg_assemble)."""
    call("bmg_assemble", out.dtype, ptr(c1), ptr(c2), ptr(rmap), i64(ashape), i64(rshape), ptr(out), stream_ptr())
    return out


def bmg_restrict(fdesc, cdesc, code, fine, out):
    """out = P^T fine over all fields (odil_bmg_transfer, mode 0); code: host c_int array, 3 per field."""
    call("bmg_transfer", out.dtype, fdesc, cdesc, code, ptr(fine), None, ptr(out), c_int(0), stream_ptr())
    return out


def bmg_prolong_add(fdesc, cdesc, code, coarse, add, out):
    """out = add + P coarse over all fields (odil_bmg_transfer, mode 1; out may be add)."""
    call("bmg_transfer", out.dtype, fdesc, cdesc, code, ptr(coarse), ptr(add), ptr(out), c_int(1), stream_ptr())
    return out


def bmg_galerkin(fdesc, cdesc, code, fcoef, ftable, ctable, nce, out):
    """Coarse coefficients P^T C P of every entry of ctable (odil_bmg_galerkin)."""
    call("bmg_galerkin", out.dtype, fdesc, cdesc, code, ptr(fcoef), ptr(ftable), ptr(ctable), c_int(nce),
         c_int64(out.numel()), ptr(out), stream_ptr())
    return out


def bmg_coarse_inverse(coef, table, desc, n, tol_rel=1e-13):
    """The coarsest level's symmetric generalised inverse, factorised on the device (odil_bmg_coarse_dense +
    odil_bmg_coarse_chol; float64).  Returns (inv: n x n, drops: device int32 per panel of 64 rows -- the dropped pivots).
    Nothing is read back."""
    assert coef.dtype == torch.float64, "the coarse factorisation is float64 only"
    npad = -(-int(n) // 64) * 64
    dev = coef.device
    work = torch.empty((npad, 2 * npad), dtype=torch.float64, device=dev)
    thr = torch.empty(1, dtype=torch.float64, device=dev)
    drops = torch.empty(npad // 64, dtype=torch.int32, device=dev)
    inv = torch.empty((int(n), int(n)), dtype=torch.float64, device=dev)
    stream = stream_ptr()
    call("bmg_coarse_dense", torch.float64, ptr(coef), ptr(table), desc, c_int64(npad), c_int64(2 * npad), ptr(work),
         stream)
    call("bmg_coarse_chol", torch.float64, ptr(work), c_int64(int(n)), c_int64(npad), float(tol_rel), ptr(thr),
         ptr(drops), ptr(inv), stream)
    return inv, drops


def bmg_coarse_dense(coef, table, desc, n):
    """The coarsest level's dense symmetric matrix 0.5 (A + A^T) on the device (odil_bmg_coarse_dense; float64, n x n)."""
    assert coef.dtype == torch.float64, "the coarse factorisation is float64 only"
    npad = -(-int(n) // 64) * 64
    out = torch.empty((npad, npad), dtype=torch.float64, device=coef.device)
    call("bmg_coarse_dense", torch.float64, ptr(coef), ptr(table), desc, c_int64(npad), c_int64(npad), ptr(out),
         stream_ptr())
    return out[:int(n), :int(n)]
