"""Members of the ensembles with several grid unknowns and node-centred axes for tests/test_fields_ensemble_gpu.py and
tests/test_fields_ensemble_host.py (a helper module, no tests):

  pair      two coupled fields u, w at a chosen location on a periodic grid: -lap u + c w - f and -lap w + u w - q, as
            plain `Field`s or with `nlvl` multigrid levels; members differ in f, q and their start (c is a Python
            number, part of the generated source: one value for all members)
  tracer    examples/velocity_from_tracer at (Nt, Nx, Ny) = (4, 8, 16): three fields at 'ncc'; members differ in the
            observed blobs (tensors: one generated source)
  tmax      examples/heat_tmax at --Nt 8 --Nx 16: a field at 'nc', then an `Array`
  constant  examples/infer_constant at --Nt 8 --Nx 16: an `Array`, then a field at 'nc'

Every member starts from its own seeded random arrays of amplitude 0.1 on EVERY level, so every gradient is non-zero from
epoch 0 on."""

import argparse
import os
import sys

import numpy as np
import torch
from conftest import ROOT

import odil_amd as odil

for sub in ("velocity_from_tracer", "heat_tmax", "infer_constant"):
    path = os.path.join(ROOT, "examples", sub)
    if path not in sys.path:
        sys.path.append(path)


def pair_operator(ctx):
    extra = ctx.extra
    ndim = ctx.domain.ndim

    def centre_and_laplacian(key):
        centre, lap = ctx.field(key), None
        for i, h in enumerate(ctx.step()):
            minus, plus = ([s if j == i else 0 for j in range(ndim)] for s in (-1, 1))
            term = (ctx.field(key, *minus) - 2 * centre + ctx.field(key, *plus)) / h ** 2
            lap = term if lap is None else lap + term
        return centre, lap

    (u, lap_u), (w, lap_w) = centre_and_laplacian("u"), centre_and_laplacian("w")
    return [("fu", extra.c * w - lap_u - extra.f), ("fw", u * w - lap_w - extra.q)]


def randomise(problem, state, seed, but=()):
    """Every array of the state but those of the keys `but`: seeded normal values of amplitude 0.1, in place."""
    rng = np.random.default_rng(seed)
    domain = problem.domain
    with torch.no_grad():
        for key, field in state.fields.items():
            for a in domain.arrays_from_field(field):
                values = 0.1 * rng.standard_normal(tuple(a.shape))
                if key not in but:
                    a.copy_(torch.as_tensor(values).to(a.dtype))
    return problem, state


def pair(cells, loc, nlvl, dtype, b, keys=("u", "w"), locs=None, kinds=None):
    """Member b of `pair` on `cells` cells with both fields at `loc`.  nlvl: levels of the MultigridFields, None: plain
    Fields.  keys: the order of the state; locs / kinds: per field another location / "plain" for a Field that stays one
    in a multigrid domain (the members the driver refuses)."""
    ndim = len(cells)
    domain = odil.Domain(cshape=list(cells), dimnames=["x", "y", "z", "s"][:ndim], multigrid=nlvl is not None, mg_nlvl=nlvl,
                         dtype=dtype)
    mod = domain.mod
    rng = np.random.default_rng(23 + 101 * b)
    shape = tuple(domain.size(loc=loc))
    extra = argparse.Namespace(c=0.75, f=mod.cast(rng.standard_normal(shape), dtype),
                               q=mod.cast(rng.standard_normal(shape), dtype))
    state = odil.State()
    for key in keys:
        state.fields[key] = odil.Field(None, loc=(locs or dict()).get(key, loc))
    state = domain.init_state(state)
    for key, kind in (kinds or dict()).items():
        if kind == "plain":
            state.fields[key] = domain.init_field(odil.Field(None, loc=(locs or dict()).get(key, loc)))
    return randomise(odil.Problem(pair_operator, domain, extra), state, 1000 + b)


def example_args(module, argv, dtype, nlvl):
    argv = list(argv) + ["--double", "1" if dtype == np.float64 else "0", "--multigrid", "0" if nlvl is None else "1"]
    if nlvl is not None:
        argv += ["--nlvl", str(nlvl)]
    return module.parse_args(argv)


def tracer(nlvl, dtype, b, cells=(4, 8, 16), kxreg=None):
    """Member b of `tracer`: the blobs it observes are shifted with b.  kxreg: another regularisation weight (a Python
    number: another generated source)."""
    import veltracer

    argv = ["--Nt", str(cells[0]), "--Nx", str(cells[1]), "--Ny", str(cells[2])]
    if kxreg is not None:
        argv += ["--kxreg", str(kxreg)]
    problem, state = veltracer.make_problem(example_args(veltracer, argv, dtype, nlvl))
    mod = problem.domain.mod
    x, y = [mod.numpy(a) for a in problem.domain.points("x", "y", loc=".cc")]
    problem.extra.u_init = mod.cast(veltracer.blob(x + 0.02 * b, y, 0), dtype)
    problem.extra.u_final = mod.cast(veltracer.blob(x, y - 0.03 * b, 1), dtype)
    return randomise(problem, state, 2000 + b)


def tmax(nlvl, dtype, b):
    import heat_tmax

    problem, state = heat_tmax.make_problem(example_args(heat_tmax, ["--Nt", "8", "--Nx", "16", "--tmax_init", str(1 + 0.25 * b)],
                                                         dtype, nlvl))
    return randomise(problem, state, 3000 + b, but=("coeff",))


def constant(nlvl, dtype, b):
    import infer_constant

    problem, state = infer_constant.make_problem(example_args(infer_constant, ["--Nt", "8", "--Nx", "16", "--c_src",
                                                                               str(0.1 + 0.05 * b)], dtype, nlvl))
    return randomise(problem, state, 4000 + b, but=("coeff",))


def run_args(optimizer="adam", epochs=6, lr=0.01, **more):
    return argparse.Namespace(optimizer=optimizer, epochs=epochs, epoch_start=0, lr=lr, **more)
