#!/usr/bin/env python3
"""Variable-coefficient diffusion in MIXED first-order form, the Darcy system

    div q = f,    q + k grad p = 0,    curl(q / k) = 0     in the unit square / cube,  p = 0 on the walls,

with the pressure p at the cells ('cc' / 'ccc') and the flux component q_i at the faces normal to axis i ('nc', 'cn';
'ncc', 'cnc', 'ccn') -- NOT one of the reference's examples: a Newton system of several coupled fields at mixed locations,
which `linsolver.solve(..., "multigrid")` takes through the multigrid for the normal equations (odil_amd/gmg.py:
NormalGMG).  The residuals are

    sum_i (q_i(+) - q_i(-)) / h - f           at the cells,
    q_i + k_i (p(+) - p(-)) / h               at the faces, p = 0 half a cell outside at the walls,
    curl(q / k)                               at the edges (`--curl 1`, the default; mirror ghosts at the walls).

The first two alone make M square and nonsingular (`--curl 0`); their least-squares functional controls q only through
its divergence, and point-smoothed multigrid loses its rate on such systems (CG iterations grow with N).  The curl rows are
satisfied by the discrete solution (the discrete gradient has no discrete curl), so the system stays consistent: one
Newton step (the least-squares solution of M d = -r) leaves the residual at round-off at any size, with or without them.

    python examples/darcy/darcy.py --ndim 2 --N 1024 --linsolver multigrid --linsolver_tol 1e-10
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import odil_amd as odil  # noqa: E402
from odil_amd import printlog  # noqa: E402

FLUX_KEYS = ("qx", "qy", "qz")


def flux_loc(ndim, i):
    return "".join("n" if j == i else "c" for j in range(ndim))


def conductivity(xx):
    """k = 1 + 0.9 prod sin(2 pi x): smooth, varies by a factor 19."""
    p = xx[0] * 0 + 1
    for x in xx:
        p = p * np.sin(2 * np.pi * x)
    return 1 + 0.9 * p


def operator(ctx):
    mod, extra = ctx.mod, ctx.extra
    ndim = ctx.domain.ndim
    h = ctx.step()
    cells = "c" * ndim
    unit = lambda i: [1 if j == i else 0 for j in range(ndim)]
    div = None
    for i in range(ndim):
        key = FLUX_KEYS[i]
        dq = ctx.field(key, *unit(i), loc=cells) - ctx.field(key, loc=cells)
        div = dq if div is None else div + dq
    res = [div / h[0] - extra.f]
    for i in range(ndim):
        loc = flux_loc(ndim, i)
        iface = ctx.indices(loc=loc)[i]
        nface = ctx.size(loc=loc)[i]
        pm = ctx.field("p", loc=loc)             # the cell below the face (0 outside the wall)
        pp = ctx.field("p", *unit(i), loc=loc)   # the cell above
        wall = mod.where((iface == 0) | (iface == nface - 1), ctx.cast(2), ctx.cast(1))  # the wall is half a cell away
        res.append(ctx.field(FLUX_KEYS[i]) + extra.kfaces[i] * (pp - pm) * wall / h[i])
    if extra.args.curl:
        res += curl_residuals(ctx)
    return res


def curl_residuals(ctx):
    """curl(q / k) = 0 at the edges (2-D: the nodes 'nn'; 3-D: the edges along each axis).  At a wall the missing
    neighbour is the mirror image of the one inside (q / k of the ghost cell = minus that of the cell inside, what p = 0
    half a cell out implies): the difference across the wall is twice the inside value.  The discrete gradient has no
    discrete curl, so the system stays consistent; the term (with its wall closure, the tangential condition) makes the
    least-squares functional control all first derivatives of q, not only its divergence."""
    mod, extra = ctx.mod, ctx.extra
    ndim = ctx.domain.ndim
    h = ctx.step()
    unit = lambda i: [1 if j == i else 0 for j in range(ndim)]
    pairs = [(0, 1)] if ndim == 2 else [(0, 1), (1, 2), (0, 2)]
    out = []
    for i, j in pairs:
        loc = "".join("n" if d in (i, j) else "c" for d in range(ndim))  # nodes along i and j, cells along the rest
        idx, size = ctx.indices(loc=loc), ctx.size(loc=loc)
        two = ctx.cast(2)
        wi = mod.where((idx[i] == 0) | (idx[i] == size[i] - 1), two, ctx.cast(1))
        wj = mod.where((idx[j] == 0) | (idx[j] == size[j] - 1), two, ctx.cast(1))
        # (a cell-centred axis read at the nodes: shift 0 is the cell below the node, shift 1 the one above, 0 outside)
        qj_m = ctx.field(FLUX_KEYS[j], loc=loc) / extra.kedge[(j, i, 0)]
        qj_p = ctx.field(FLUX_KEYS[j], *unit(i), loc=loc) / extra.kedge[(j, i, 1)]
        qi_m = ctx.field(FLUX_KEYS[i], loc=loc) / extra.kedge[(i, j, 0)]
        qi_p = ctx.field(FLUX_KEYS[i], *unit(j), loc=loc) / extra.kedge[(i, j, 1)]
        out.append((qj_p - qj_m) * wi / h[i] - (qi_p - qi_m) * wj / h[j])
    return out


def make_problem(args):
    dtype = np.float64 if args.double else np.float32
    ndim = args.ndim
    domain = odil.Domain(cshape=[args.N] * ndim, dimnames=["x", "y", "z"][:ndim], multigrid=0, dtype=dtype)
    mod = domain.mod
    kfaces = []
    for i in range(ndim):
        xx = [mod.numpy(a) for a in domain.points(loc=flux_loc(ndim, i))]
        kfaces.append(mod.cast(conductivity(xx), dtype))
    xx = [mod.numpy(a) for a in domain.points(loc="c" * ndim)]
    f = mod.cast(np.ones_like(xx[0]) + xx[0], dtype)
    # k of the faces next to every edge: (component, axis of the step, side)
    kedge = dict()
    if args.curl:
        pairs = [(0, 1)] if ndim == 2 else [(0, 1), (1, 2), (0, 2)]
        step = [float(v) for v in domain.step()]
        for i, j in pairs:
            loc = "".join("n" if d in (i, j) else "c" for d in range(ndim))
            pts = [mod.numpy(a) for a in domain.points(loc=loc)]
            for comp, ax in ((j, i), (i, j)):
                for side, sh in ((0, -0.5), (1, 0.5)):
                    xx = [x + (sh * step[ax] if d == ax else 0.0) for d, x in enumerate(pts)]
                    kedge[(comp, ax, side)] = mod.cast(conductivity(xx), dtype)
    state = odil.State()
    state.fields["p"] = odil.Field(None, loc="c" * ndim)
    for i in range(ndim):
        state.fields[FLUX_KEYS[i]] = odil.Field(None, loc=flux_loc(ndim, i))
    state = domain.init_state(state)
    extra = argparse.Namespace(kfaces=kfaces, kedge=kedge, f=f, args=args)
    return odil.Problem(operator, domain, extra), state


def parse_args(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--ndim", type=int, choices=[2, 3], default=2, help="Space dimension")
    parser.add_argument("--N", type=int, default=64, help="Cells per axis")
    parser.add_argument("--curl", type=int, default=1, help="Add the residuals curl(q / k) = 0 at the edges (0: M is square)")
    odil.util.add_arguments(parser)
    odil.linsolver.add_arguments(parser)
    parser.set_defaults(frames=1, report_every=1, history_every=1, plot_every=1, history_full=50)
    parser.set_defaults(optimizer="newton", multigrid=0, double=1, epochs=1, outdir="out_darcy", linsolver="multigrid")
    return parser.parse_args(argv)


def main():
    args = parse_args()
    odil.setup_outdir(args)
    problem, state = make_problem(args)
    callback = odil.make_callback(problem, args)
    odil.util.optimize(args, args.optimizer, problem, state, callback)


if __name__ == "__main__":
    main()
