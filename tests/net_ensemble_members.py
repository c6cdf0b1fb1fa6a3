"""Members of the ensembles of inverse problems with `NeuralNet` unknowns and priors, for tests/test_net_ensemble_gpu.py and
tests/test_net_ensemble_host.py (a helper module, no tests).

The operators are those of examples/heat/heat.py and heat2d.py with the arguments of the committed fixtures
(tests/golden/heat_f64.npz: 8 x 16 cells, 3 levels; heat2d_f64.npz: 8 x 8 x 16, 3 levels), a [1, 5, 5, 1] network `k_net`
beside the field `u`.  heat's own `wreg` is `(stop_gradient(ww) - ww) k`: identically zero with zero gradient, so it says
nothing about the parameter kernel.  `live_operator` therefore adds terms that do not vanish:

  wdecay   ww * k, k annealed with the `epoch` tracer (a host scalar of the parameter kernel);
  cprior   (c - 0.3) * kc on an `Array` c of four elements beside the network, of which the grid residual reads c[0]
           (its gradient has a grid part and a prior part) and nothing reads c[1:] but the prior.

`frozen_operator` reads its network only with frozen=True and regularises it: no grid kernel writes the gradient of its
weights, the parameter kernel SETS it.

Members differ in seed (imposed points, network, start), in the weight of the imposed points (the mask is scaled: what
another `kimp` does) and in the weights `kdecay` and `kc` of the priors, which are TRACERS of the member's problem: a Python
number in the operator is part of the generated source, and members with different sources run as groups of their own
(the test of the groups), while tensors and tracers leave all members in one group."""

import argparse
import os
import sys

import numpy as np
from conftest import ROOT

import odil_amd as odil
from odil_amd import param_expr, stencil_jit
from odil_amd.stencil_bind import field_ranges
from odil_amd.stencil_codegen import _Codegen

FIXTURE = ["--infer_k", "1", "--kimp", "2", "--kxreg", "0.3", "--kxregdecay", "50", "--ktreg", "0.2", "--ktregdecay", "0",
           "--imposed", "stripe", "--nimp", "40"]
SHAPES = dict(heat=(8, 16), heat2d=(8, 8, 16), plain=(12, 18))
FORMS = dict(heat="launches", heat2d="volumes", plain="launches")
ARCH = (5, 5)


def example(which):
    path = os.path.join(ROOT, "examples", "heat")
    if path not in sys.path:
        sys.path.insert(0, path)
    return __import__("heat2d" if which == "heat2d" else "heat")


def heat_args(which, dtype, b=0, kwreg=0.05):
    """The arguments of the fixtures for member b (its seed); which = "plain": 12 x 18, --multigrid 0."""
    shape = SHAPES[which]
    argv = ["--Nt", str(shape[0]), "--Nx", str(shape[1])] + (["--Ny", str(shape[2])] if len(shape) == 3 else []) + FIXTURE
    if which != "heat2d":  # (heat2d has no weight regulariser)
        argv += ["--kwreg", repr(kwreg), "--kwregdecay", "10"]
    argv += ["--seed", str(b), "--double", "1" if dtype == np.float64 else "0", "--multigrid", "0" if which == "plain" else "1"]
    return example(which).parse_args(argv)


def network(rng, arch, ninputs=1):
    layers = [ninputs] + list(arch) + [1]
    weights = [rng.uniform(-1, 1, (no, ni)) / np.sqrt(ni) for ni, no in zip(layers[:-1], layers[1:])]
    biases = [0.1 * rng.standard_normal(no) for no in layers[1:]]
    return odil.NeuralNet(weights, biases)


def live_operator(ctx):
    """The heat operator with c[0] in its residual, a weight decay annealed with the epoch and a prior on c."""
    extra, mod = ctx.extra, ctx.mod
    res = example("heat2d" if ctx.domain.ndim == 3 else "heat").operator(ctx)
    res[0] = (res[0][0], res[0][1] * (1 + 0.1 * ctx.field("c")[0]))
    ww = ctx.domain.arrays_from_field(ctx.state.fields["k_net"])
    flat = mod.concatenate([mod.flatten(w) for w in ww], axis=0)
    res.append(("wdecay", flat * (ctx.tracers["kdecay"] * 0.5 ** (ctx.tracers["epoch"] / 4))))
    c = ctx.domain.arrays_from_field(ctx.state.fields["c"])[0]
    res.append(("cprior", (c - 0.3) * ctx.tracers["kc"]))
    return res


def constant_prior_operator(ctx):
    """heat with a weight decay that no tracer anneals and no annealed grid term either: no host scalars."""
    mod = ctx.mod
    res = example("heat").operator(ctx)
    ww = ctx.domain.arrays_from_field(ctx.state.fields["k_net"])
    res.append(("wdecay", mod.concatenate([mod.flatten(w) for w in ww], axis=0) * ctx.extra.kdecay))
    return res


def torch_replayed_operator(ctx):
    """A reduction of a weight matrix has no elementwise form: only the torch replay evaluates this output."""
    res = example("heat").operator(ctx)
    ww = ctx.domain.arrays_from_field(ctx.state.fields["k_net"])
    return res + [("wsum", ww[0].sum().reshape(1) * 0.1)]


def frozen_operator(ctx):
    """u_t = k(u) u_xx + q on a periodic (t, x) grid, k = sigmoid(net(u)) read with frozen=True, and a weight decay."""
    extra, mod = ctx.extra, ctx.mod
    dt, dx = ctx.step()
    u, uo, um, up = ctx.field("u"), ctx.field("u", -1, 0), ctx.field("u", 0, -1), ctx.field("u", 0, 1)
    k = mod.sigmoid(ctx.neural_net("k_net", frozen=True)(ctx.field("u", frozen=True))[0]) * 0.1
    fu = (u - uo) / dt - k * (up - 2 * u + um) / (dx * dx) - extra.q
    ww = ctx.domain.arrays_from_field(ctx.state.fields["k_net"])
    flat = mod.concatenate([mod.flatten(w) for w in ww], axis=0)
    return [("fu", fu), ("wdecay", flat * (ctx.tracers["kdecay"] * 0.5 ** (ctx.tracers["epoch"] / 4)))]


OPERATORS = dict(heat=None, live=live_operator, constant=constant_prior_operator, torch=torch_replayed_operator,
                 frozen=frozen_operator)


def make_member(which, dtype, b, operator="heat", order="after", arch=ARCH, annealed=True, activation=None):
    """Member b.  which: "heat", "heat2d" or "plain" (`SHAPES`).  operator: a key of `OPERATORS` ("heat": the example's
    own).  order: "after" (u, k_net[, c]) or "before" (k_net[, c], u).  annealed=False: without the terms annealed with the
    epoch (kxregdecay = kwregdecay = 0): no host scalars.  activation: of the network (default tanh)."""
    ex = example(which)
    args = heat_args(which, dtype, b)
    if not annealed:
        args.kxregdecay, args.kwregdecay = 0, 0
    problem, _ = ex.make_problem(args)
    domain, extra = problem.domain, problem.extra
    rng = np.random.default_rng(1000 + 17 * b)
    extra.kdecay = 0.05
    extra.imp_mask = extra.imp_mask * (1 + 0.25 * b)
    extra.q = domain.mod.cast(rng.standard_normal(domain.cshape), dtype)
    fields = dict(u=0.05 * rng.standard_normal(domain.cshape), k_net=network(rng, arch))
    fields["k_net"].activation = activation or "tanh"
    keys = ["u", "k_net"]
    if operator == "live":
        fields["c"] = odil.Array(np.array([0.5, -0.2, 0.1, 0.8]) + 0.05 * rng.standard_normal(4))
        keys.append("c")
    if order == "before":
        keys = keys[1:] + keys[:1]
    state = domain.init_state(odil.State(fields={key: fields[key] for key in keys}))
    tracers = {"epoch": 0, "kdecay": 0.05 * (1 + b), "kc": 0.5 + 0.25 * b}
    return odil.Problem(OPERATORS[operator] or ex.operator, domain, extra, tracers=tracers), state


def make_members(which, dtype, nb, **kwargs):
    built = [make_member(which, dtype, b, **kwargs) for b in range(nb)]
    return [p for p, _ in built], [s for _, s in built]


def run_args(optimizer="adam", epochs=6, lr=0.01, **more):
    return argparse.Namespace(optimizer=optimizer, epochs=epochs, epoch_start=0, lr=lr, **more)


def advance_epoch(problem, epoch):
    """What the callbacks of both sides do: the next evaluation sees the epoch it belongs to."""
    problem.tracers["epoch"] = epoch + 1


def generate(problem, state, batch):
    """(cg, source) as `stencil_bind.StencilBinding` generates them: with the outputs in parameter space handed to the
    generator in their elementwise form (`k_par`)."""
    from odil_amd.core import Array, NeuralNet

    domain = problem.domain
    tr, outs, raw, names, G = stencil_jit.trace_outputs(problem, state)
    cg = _Codegen(tr, outs, raw, G, state, batch=batch)
    offgrid = [(k, e, tr.param_tape.slice_for(e.param_ids())) for k, e in tr.offgrid]
    if offgrid:
        numel = {i: int(a.numel()) for i, a in enumerate(domain.arrays_from_state(state))}
        cg.parameter_outputs(param_expr.convert(tr.param_tape, offgrid, numel), numel, {
            i: key for key, field, pos, n in field_ranges(domain, state) if isinstance(field, (NeuralNet, Array))
            for i in range(pos, pos + n)})
    return cg, cg.source()
