"""Float64 CPU reference for the Jacobian of an operator on plain grid fields (TEST INFRASTRUCTURE): the operator is run
on torch CPU tensors through the oracle's `Context` (oracle/odil_generic.py, pinned against fixtures the reference
produced) and differentiated by torch autograd as ONE function from the fields to the concatenated outputs -- nothing here
knows about shifts, reads or coefficient arrays.  The other half turns what `Problem.eval_operator_grad` returns (per output
a dict {(key, shift, loc): array}) into the matrix it stands for, so that the two can be compared entry by entry.

Conventions: rows follow the outputs in order, each flattened in C order; columns follow `keys` (the state's field order),
each field flattened in C order.  Everything is float64 whatever the domain's dtype; fields are cell-centred."""

import numpy as np
import torch

from oracle import odil_generic as og


def _geometry(domain):
    geom = og.Geometry.of(domain)
    if np.dtype(geom.dtype) != np.float64:  # a float32 problem: its reference is the float64 evaluation of the same operator
        geom = og.Geometry(geom.cshape, geom.dimnames, np.asarray(domain.lower, dtype=np.float64),
                           np.asarray(domain.upper, dtype=np.float64), np.float64)
    return geom


def _function(operator, domain, arrays, extra):
    """(f, inputs, keys): f maps the field arrays (in the order of `arrays`) to the list of the operator's outputs."""
    geom = _geometry(domain)
    keys = list(arrays)
    inputs = tuple(torch.as_tensor(np.asarray(arrays[k]), dtype=torch.float64).clone() for k in keys)
    for t in inputs:
        assert tuple(t.shape) == geom.cshape, "cell-centred fields on the whole grid only"
    if extra is not None and not isinstance(extra, torch.Tensor):
        extra = torch.as_tensor(np.asarray(extra), dtype=torch.float64)
    if isinstance(extra, torch.Tensor):
        extra = extra.detach().cpu().to(torch.float64)
    locs = {k: "c" * geom.ndim for k in keys}

    def f(*xs):
        ctx = og.Context(geom, dict(zip(keys, xs)), locs, dict(), extra, dict(epoch=0))
        _, values = og.split_outputs(operator(ctx))
        return values

    return f, inputs, keys


def values(operator, domain, arrays, extra=None):
    """The operator's outputs (list of float64 arrays)."""
    f, inputs, _ = _function(operator, domain, arrays, extra)
    with torch.no_grad():
        return [v.numpy().copy() for v in f(*inputs)]


def dense_jacobian(operator, domain, arrays, extra=None):
    """d (concatenated outputs) / d (concatenated fields) as a dense float64 matrix, by reverse-mode autograd."""
    f, inputs, _ = _function(operator, domain, arrays, extra)
    flat = lambda *xs: torch.cat([v.reshape(-1) for v in f(*xs)])
    blocks = torch.autograd.functional.jacobian(flat, inputs, vectorize=True)
    return torch.cat([b.reshape(b.shape[0], -1) for b in blocks], dim=1).numpy()


def jvp(operator, domain, arrays, v, extra=None):
    """J v for v: key -> array (the fields' shapes); the concatenated outputs' layout."""
    f, inputs, keys = _function(operator, domain, arrays, extra)
    flat = lambda *xs: torch.cat([o.reshape(-1) for o in f(*xs)])
    vs = tuple(torch.as_tensor(np.asarray(v[k]), dtype=torch.float64) for k in keys)
    return torch.autograd.functional.jvp(flat, inputs, vs)[1].numpy()


def vjp(operator, domain, arrays, y, extra=None):
    """J^T y for y in the concatenated outputs' layout; the concatenated fields' layout."""
    f, inputs, _ = _function(operator, domain, arrays, extra)
    flat = lambda *xs: torch.cat([o.reshape(-1) for o in f(*xs)])
    res = torch.autograd.functional.vjp(flat, inputs, torch.as_tensor(np.asarray(y), dtype=torch.float64))[1]
    return torch.cat([r.reshape(-1) for r in res]).numpy()


def _np64(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def columns(shift, G):
    """Flat index of the point (p + shift) mod G for every point p of the grid, in C order: what `ctx.field(key, *shift)`
    shows at p (a periodic roll by -shift: oracle/odil_generic.field_access)."""
    idx = np.meshgrid(*[(np.arange(g) + s) % g for g, s in zip(G, shift)], indexing="ij")
    return np.ravel_multi_index(idx, G).reshape(-1)


def _entries(grads, G):
    """(output position, key, shift, flat coefficient array) of every array of `grads`; None arrays (the autograd route's
    reads an output does not depend on) are skipped."""
    n = int(np.prod(G))
    for k, grad in enumerate(grads):
        for (key, shift, loc), a in grad.items():
            if a is None:
                continue
            assert loc == "c" * len(G) and len(shift) == len(G), (key, shift, loc)
            a = _np64(a)
            assert a.size == n, "one coefficient per row: {} has shape {} on grid {}".format((key, shift, loc), a.shape, G)
            yield k, key, tuple(int(s) for s in shift), a.reshape(-1)


def assemble(values, grads, keys, G):
    """The dense matrix that per-output dicts {(key, shift, loc): array} stand for: row p of output k gets array[p] at the
    column of `key` at (p + shift) mod G; entries that land on one column add up."""
    n, G = int(np.prod(G)), tuple(G)
    assert len(values) == len(grads) and all(int(np.prod(v.shape)) == n for v in values)
    M = np.zeros((len(grads) * n, len(keys) * n))
    rows = np.arange(n)
    for k, key, shift, a in _entries(grads, G):
        np.add.at(M, (k * n + rows, keys.index(key) * n + columns(shift, G)), a)
    return M


def apply(values, grads, keys, G, v):
    """The same matrix times v (key -> array), without forming it."""
    n, G = int(np.prod(G)), tuple(G)
    y = np.zeros(len(grads) * n)
    for k, key, shift, a in _entries(grads, G):
        y[k * n:(k + 1) * n] += a * _np64(v[key]).reshape(-1)[columns(shift, G)]
    return y


def apply_transposed(values, grads, keys, G, y):
    """The transposed matrix times y (the concatenated outputs' layout): the concatenated fields' layout."""
    n, G = int(np.prod(G)), tuple(G)
    y = _np64(y).reshape(-1)
    x = np.zeros(len(keys) * n)
    for k, key, shift, a in _entries(grads, G):
        np.add.at(x, keys.index(key) * n + columns(shift, G), a * y[k * n:(k + 1) * n])
    return x


def check_pairs(grads, J, keys, G):
    """The set of keys is the Jacobian's structure: an output whose block of the dense reference `J` for a field is not
    zero has at least one array for that field, and an array with a nonzero entry belongs to a nonzero block.  (An array of
    zeros beside a zero block is no mislabelling: the symbolic derivative keeps a read behind a branch that this grid and
    state never take -- an index mask that is empty on three rows, a clip that saturates everywhere.)"""
    n = int(np.prod(G))
    for k, grad in enumerate(grads):
        for c, key in enumerate(keys):
            labels = sorted((kk, shift) for (kk, shift, loc), a in grad.items() if kk == key and a is not None)
            live = [(kk, shift) for kk, shift in labels if np.any(_np64(grad[(kk, shift, "c" * len(G))]) != 0)]
            nonzero = bool(np.any(J[k * n:(k + 1) * n, c * n:(c + 1) * n] != 0))
            assert labels or not nonzero, "output {}, field '{}': no array, but the reference block is nonzero".format(k, key)
            assert nonzero or not live, "output {}, field '{}': arrays {} but the reference block is zero".format(k, key, live)
