"""Members and layouts of the ensembles of 4-D members for tests/test_members4d_gpu.py and tests/test_members4d_host.py (a
helper module, no tests):

  tracer3d  examples/velocity_from_tracer/veltracer3d.py at cells (Nt, Nx, Ny, Nz) = (8, 8, 8, 8): four fields u, vx, vy, vz
            at 'nccc' on (t, x, y, z); members differ in the observed blobs (tensors: one generated source).  (The
            `Domain` plans two levels for 4 time cells -- no coarse extent below 2 --; with 8 it plans three, TRACER3D_LEVELS:
            a node-centred marching level and a fast one)
  cell4     ONE unknown at 'cccc' on a (t, x, y, z) grid: u - k lap u - f with a 4-D Laplacian; members differ in f
  cell4_array  the same with an `Array` of two constants AFTER the field: c[0] u - c[1] lap u - f
  net4      ONE unknown at 'cccc' beside a pointwise `NeuralNet`: u_t - div(k grad u) on the last two axes with the
            conductivity k = sigmoid(net(u)) at the faces, evaluated on frozen values (the pattern of examples/heat); in
            float32 with a last axis of 128 cells or more its forward kernel is the MARCHING one

Every member starts from its own seeded random arrays of amplitude 0.1 on EVERY level (`fields_ensemble_members.randomise`)."""

import argparse

import numpy as np
from fields_ensemble_members import example_args, randomise

import odil_amd as odil

# (location, level shapes of one row, the transposed prolongation a single row runs per level >= 1:
#  0 generic, 1 fast, 2 node-centred marching -- odil_interp_adj_kind)
GENERIC, FAST, NODE = 0, 1, 2
LAYOUTS4 = [
    ("nccc", [(5, 8, 8, 8), (3, 4, 4, 4), (2, 2, 2, 2)], [NODE, FAST]),  # coarse rows of 16 elements on the fast level
    ("nccc", [(5, 8, 8, 16), (3, 4, 4, 8)], [NODE]),  # float rows wide enough for two columns per thread
    ("cccc", [(8, 8, 8, 8), (4, 4, 4, 4), (2, 2, 2, 2)], [FAST, FAST]),
    ("cccn", [(4, 4, 4, 5), (2, 2, 2, 3)], [GENERIC]),
    ("ccnc", [(4, 4, 5, 4), (2, 2, 3, 2)], [GENERIC]),
]
LAYOUT_IDS = ["{}-{}".format(loc, "x".join(map(str, shapes[0]))) for loc, shapes, _ in LAYOUTS4]


def kinds_of(lib, i64, loc, shapes, elem_size):
    return [lib.odil_interp_adj_kind(i64(list(s)), len(s), loc.encode(), elem_size) for s in shapes[1:]]


TRACER3D_LEVELS = [(9, 8, 8, 8), (5, 4, 4, 4), (3, 2, 2, 2)]


def tracer3d(nlvl, dtype, b, cells=(8, 8, 8, 8), kxreg=None):
    """Member b of `tracer3d`: the blobs it observes are shifted with b.  nlvl: multigrid levels, None: plain Fields.  kxreg:
    another regularisation weight (a Python number: another generated source)."""
    import veltracer3d

    argv = ["--Nt", str(cells[0]), "--Nx", str(cells[1]), "--Ny", str(cells[2]), "--Nz", str(cells[3])]
    if kxreg is not None:
        argv += ["--kxreg", str(kxreg)]
    problem, state = veltracer3d.make_problem(example_args(veltracer3d, argv, dtype, nlvl))
    domain = problem.domain
    x, y, z = np.meshgrid(*domain.points_1d("x", "y", "z"), indexing="ij")
    problem.extra.u_init = domain.mod.cast(veltracer3d.blob(x + 0.02 * b, y, z, 0), dtype)
    problem.extra.u_final = domain.mod.cast(veltracer3d.blob(x, y - 0.03 * b, z, 1), dtype)
    return randomise(problem, state, 5000 + b)


def cell4_operator(ctx):
    extra = ctx.extra
    u, lap = ctx.field("u"), None
    for i, h in enumerate(ctx.step()):
        minus, plus = ([s if j == i else 0 for j in range(4)] for s in (-1, 1))
        term = (ctx.field("u", *minus) - 2 * u + ctx.field("u", *plus)) / h ** 2
        lap = term if lap is None else lap + term
    if extra.with_array:
        c = ctx.field("coeff")
        return [("fu", c[0] * u - c[1] * lap - extra.f)]
    return [("fu", u - extra.k * lap - extra.f)]


def cell4(nlvl, dtype, b, cells=(8, 8, 8, 8), with_array=False):
    """Member b of `cell4` (with_array: of `cell4_array`) on `cells` cells with `nlvl` multigrid levels (None: a plain Field)."""
    domain = odil.Domain(cshape=list(cells), dimnames=["t", "x", "y", "z"], multigrid=nlvl is not None, mg_nlvl=nlvl, dtype=dtype)
    rng = np.random.default_rng(61 + 101 * b)
    extra = argparse.Namespace(k=0.01, with_array=with_array, f=domain.mod.cast(rng.standard_normal(tuple(cells)), dtype))
    state = odil.State()
    state.fields["u"] = odil.Field(None, loc="cccc")
    if with_array:
        state.fields["coeff"] = odil.Array([1.0 + 0.1 * b, 0.01])
    state = domain.init_state(state)
    return randomise(odil.Problem(cell4_operator, domain, extra), state, 6000 + b, but=("coeff",))


def net4_operator(ctx):
    mod, steps = ctx.mod, ctx.step()
    u, f = ctx.field("u"), ctx.field("u", frozen=True)
    fu = (u - ctx.field("u", -1, 0, 0, 0)) / steps[0]
    net = ctx.neural_net("k_net")
    for a in (2, 3):
        minus, plus = ([s if j == a else 0 for j in range(4)] for s in (-1, 1))
        m, p = ctx.field("u", *minus), ctx.field("u", *plus)
        fm, fp = ctx.field("u", *minus, frozen=True), ctx.field("u", *plus, frozen=True)
        k_m, k_p = mod.sigmoid(net((f + fm) * 0.5)[0]), mod.sigmoid(net((fp + f) * 0.5)[0])
        fu = fu - ((p - u) * k_p - (u - m) * k_m) / steps[a] ** 2
    return [("fu", fu)]


def net4(dtype, b, cells=(2, 4, 16, 128)):
    """Member b of `net4` on `cells` cells: a plain Field at 'cccc' and a network of layers 1-5-5-1."""
    domain = odil.Domain(cshape=list(cells), dimnames=["t", "x", "y", "z"], dtype=dtype)
    state = odil.State()
    state.fields["u"] = odil.Field(None, loc="cccc")
    state.fields["k_net"] = domain.make_neural_net([1, 5, 5, 1])
    state = domain.init_state(state)
    return randomise(odil.Problem(net4_operator, domain, argparse.Namespace()), state, 8000 + b, but=("k_net",))
