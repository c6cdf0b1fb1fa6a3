"""Members of the ensembles of inverse problems for tests/test_param_ensemble_gpu.py and tests/test_param_ensemble_host.py
(a helper module, no tests): the operator of examples/diffusion/infer.py on grids of any extents and level counts with a
third constant (a reaction term), optionally a second `Array` of shape (2, 2) that scales the two outputs, the `Array`s
before or after the field in the state.  Members differ in noise, mask, data weight and the fields p, q (all seeded);
every member starts with its constants at half their true values."""

import argparse
import os
import sys

import numpy as np
from conftest import ROOT

import odil_amd as odil

TRUE = np.array([1.0, 2.0, 0.5])  # a*, s*, r*
MIX = np.array([[1.0, 0.25], [0.5, 2.0]])  # the start of the second Array: (1 + 0.1 mix[0, 1]) eq, (1 + 0.1 mix[1, 0]) data


def diffusion():
    path = os.path.join(ROOT, "examples", "diffusion")
    if path not in sys.path:
        sys.path.append(path)
    import diffusion as module

    return module


def operator(ctx):
    """div((1 + c0 p) grad u) - c1 q - c2 u and the weighted data misfit; with a second Array `mix` (2, 2) in the state,
    the outputs times 1 + 0.1 mix[0, 1] and 1 + 0.1 mix[1, 0] (two of its four elements are never read: zero gradient)."""
    mod, extra = ctx.mod, ctx.extra
    dirs = range(ctx.domain.ndim)
    c = ctx.field("coeff")
    st = [ctx.field("u")]
    for i in dirs:
        st.append(ctx.field("u", *[-1 if j == i else 0 for j in dirs]))
        st.append(ctx.field("u", *[1 if j == i else 0 for j in dirs]))
    kfaces = [tuple(1 + c[0] * p for p in pair) for pair in extra.pfaces]
    fu = diffusion().flux_divergence(st, kfaces, dirs, ctx.indices(), ctx.size(), ctx.step(), mod)
    fu = fu - c[1] * extra.q - extra.reaction * c[2] * st[0]
    data = extra.wmask * (st[0] - extra.u_obs)
    if extra.mix:
        mix = ctx.field("mix")
        fu, data = (1 + 0.1 * mix[0, 1]) * fu, (1 + 0.1 * mix[1, 0]) * data
    return [("eq", fu), ("data", data)]


def forward_only(ctx):
    """The same equation with the constants given: a member WITHOUT Array unknowns."""
    mod, extra = ctx.mod, ctx.extra
    dirs = range(ctx.domain.ndim)
    st = [ctx.field("u")]
    for i in dirs:
        st.append(ctx.field("u", *[-1 if j == i else 0 for j in dirs]))
        st.append(ctx.field("u", *[1 if j == i else 0 for j in dirs]))
    kfaces = [tuple(1 + p for p in pair) for pair in extra.pfaces]
    return [diffusion().flux_divergence(st, kfaces, dirs, ctx.indices(), ctx.size(), ctx.step(), mod) - extra.q]


def make_member(cshape, nlvl, dtype, b, order="after", mix=False, operator_=None, coeff_shape=(3,), reaction=1.0):
    """Member b on cells `cshape`.  nlvl: levels of the MultigridField unknown, None: a plain Field.  order: "after" (u,
    coeff[, mix]), "before" (coeff[, mix], u) or "around" (mix, u, coeff).  coeff_shape: of the first Array (the operator
    reads elements 0 ... 2).  reaction: a Python constant in front of the reaction term (another value: another source)."""
    dif = diffusion()
    ndim = len(cshape)
    domain = odil.Domain(cshape=list(cshape), dimnames=["x", "y", "z"][:ndim], multigrid=nlvl is not None, mg_nlvl=nlvl, dtype=dtype)
    mod = domain.mod
    x1 = [np.asarray(mod.numpy(x), dtype=np.float64) for x in domain.points_1d()]
    step = [float(s) for s in domain.step()]
    rng = np.random.default_rng(11 + 101 * b)
    amp = 0.5 + 0.5 * rng.random()
    pfaces = []
    for i in range(ndim):
        pair = []
        for sign in (-0.5, 0.5):
            coords = [x + (sign * step[i] if j == i else 0.0) for j, x in enumerate(x1)]
            pair.append(mod.cast(amp * (dif.conductivity("smooth", np.meshgrid(*coords, indexing="ij")) - 1), dtype))
        pfaces.append(tuple(pair))
    ref = dif.reference_solution(np.meshgrid(*x1, indexing="ij"))
    q = mod.cast(-(1.0 + rng.random()) * ref * (np.pi ** 2) * ndim, dtype)
    u_obs = mod.cast(ref + 0.01 * rng.standard_normal(ref.shape), dtype)
    wmask = mod.cast((1.0 + b) * (rng.random(ref.shape) < 0.5), dtype)
    coeff = np.zeros(coeff_shape)
    coeff.reshape(-1)[:3] = 0.5 * TRUE
    fields = dict(u=0.5 * ref + 0.05 * rng.standard_normal(ref.shape))
    if operator_ is not forward_only:
        fields["coeff"] = odil.Array(coeff)
        if mix:
            fields["mix"] = odil.Array(MIX.copy())
    keys = dict(after=["u", "coeff", "mix"], before=["coeff", "mix", "u"], around=["mix", "u", "coeff"])[order]
    state = odil.State(fields={key: fields[key] for key in keys if key in fields})
    state = domain.init_state(state)
    extra = argparse.Namespace(pfaces=pfaces, q=q, u_obs=u_obs, wmask=wmask, mix=bool(mix), reaction=float(reaction))
    return odil.Problem(operator_ or operator, domain, extra), state


def make_members(cshape, nlvl, dtype, nb, **kwargs):
    built = [make_member(cshape, nlvl, dtype, b, **kwargs) for b in range(nb)]
    return [p for p, _ in built], [s for _, s in built]


def run_args(optimizer="adam", epochs=6, lr=0.01, **more):
    return argparse.Namespace(optimizer=optimizer, epochs=epochs, epoch_start=0, lr=lr, **more)
