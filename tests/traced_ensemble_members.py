"""Members of the traced Adam ensembles for tests/test_traced_ensemble_gpu.py and tests/test_traced_ensemble_host.py (a
helper module, no tests): the operator of examples/diffusion/ensemble.py on grids of any extents and level counts, members
that differ in conductivity amplitude, right-hand side and initial guess (all seeded), and an operator with two outputs."""

import argparse
import importlib.util
import os
import sys

import numpy as np
from conftest import ROOT

import odil_amd as odil


def diffusion_ensemble():
    """examples/diffusion/ensemble.py under a name of its own (examples/poisson has an `ensemble` module too)."""
    name = "diffusion_ensemble_example"
    if name not in sys.modules:
        path = os.path.join(ROOT, "examples", "diffusion")
        if path not in sys.path:
            sys.path.append(path)  # (for its `import diffusion`)
        spec = importlib.util.spec_from_file_location(name, os.path.join(path, "ensemble.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


def two_outputs(ctx):
    """The residual of the example's operator and, with another weight, a penalty on the x-difference of u: two outputs,
    so `k_final` / `k_loss` sum two rows of partials and the loss has two terms."""
    fu = diffusion_ensemble().operator(ctx)[0]
    shift = [1] + [0] * (ctx.domain.ndim - 1)
    return [fu, 0.25 * (ctx.field("u", *shift) - ctx.field("u"))]


def make_member(cshape, nlvl, dtype, b, nb, beta=0.0, operator=None, seed=7, mg_factors=None):
    """Member b of nb on cells `cshape`: conductivity 1 + a_b (k - 1), a_b = (b + 1) / nb, a right-hand side and an
    initial guess of its own (seeded by b).  nlvl: levels of the MultigridField unknown, None: a plain Field."""
    example = diffusion_ensemble()
    diffusion = sys.modules["diffusion"]
    ndim = len(cshape)
    domain = odil.Domain(cshape=list(cshape), dimnames=["x", "y", "z"][:ndim], multigrid=nlvl is not None, mg_nlvl=nlvl,
                         mg_factors=mg_factors, dtype=dtype)
    mod = domain.mod
    x1 = [np.asarray(mod.numpy(x), dtype=np.float64) for x in domain.points_1d()]
    step = [float(s) for s in domain.step()]
    amp = (b + 1) / nb
    kfaces = []
    for i in range(ndim):
        pair = []
        for sign in (-0.5, 0.5):
            coords = [x + (sign * step[i] if j == i else 0.0) for j, x in enumerate(x1)]
            k = diffusion.conductivity("smooth", np.meshgrid(*coords, indexing="ij"))
            pair.append(mod.cast(1 + amp * (k - 1), dtype))
        kfaces.append(tuple(pair))
    rng = np.random.default_rng(seed + 101 * b)
    rhs = mod.cast(rng.standard_normal(cshape), dtype)
    state = odil.State()
    state.fields["u"] = 0.1 * rng.standard_normal(cshape)
    state = domain.init_state(state)
    extra = argparse.Namespace(rhs=rhs, kfaces=kfaces, beta=float(beta), args=argparse.Namespace(sigma=0.0))
    return odil.Problem(operator or example.operator, domain, extra), state


def make_members(cshape, nlvl, dtype, nb, beta=0.0, **kwargs):
    """beta: one value, or one per member."""
    betas = list(beta) if isinstance(beta, (list, tuple)) else [beta] * nb
    built = [make_member(cshape, nlvl, dtype, b, nb, beta=betas[b], **kwargs) for b in range(nb)]
    return [p for p, _ in built], [s for _, s in built]


def run_args(epochs=3, lr=0.01):
    return argparse.Namespace(optimizer="adam", epochs=epochs, epoch_start=0, lr=lr)
