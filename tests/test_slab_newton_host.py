"""Newton on the slab decomposition, host side (no GPU): what `slab_solvers.check_slab_newton` refuses, decided on CPU
tensors from the generated Jacobian kernel's `jac_items` traced on the host (as build() traces), and the mapping of a
Jacobian's per-shift arrays to the [7, ...] coefficient layout of the multigrid solvers (`gmg.stencil_coefficients`)."""

import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
sys.path.insert(0, os.path.join(ROOT, "examples", "darcy"))


@pytest.fixture(autouse=True)
def cpu_mod():
    import odil_amd as odil
    from odil_amd import runtime

    saved, saved_log = runtime._mod, odil.util.g_log_file
    runtime._mod = odil.ModRocm(device="cpu")
    odil.util.set_log_file(open(os.devnull, "w"))
    yield
    runtime._mod = saved
    odil.util.g_log_file = saved_log


def diffusion(*argv):
    import diffusion as ex

    args = ex.parse_args(["--ndim", "3", "--N", "16", "--kind", "jump"] + list(argv))
    problem, state = ex.make_problem(args)
    return args, problem, state


def check(args, problem, state, **kw):
    from odil_amd.slab_solvers import check_slab_newton

    return check_slab_newton(args, problem, state, **kw)


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("linsolver", ["multigrid", "direct"])
def test_admits_diffusion(world, linsolver):
    args, problem, state = diffusion("--linsolver", linsolver, "--sigma", "1")
    assert check(args, problem, state, world=world) is None


def test_refuses_2d():
    import diffusion as ex

    args = ex.parse_args(["--ndim", "2", "--N", "16"])
    problem, state = ex.make_problem(args)
    with pytest.raises(NotImplementedError, match="2-D"):
        check(args, problem, state)


def test_refuses_other_cut_axis():
    args, problem, state = diffusion()
    with pytest.raises(NotImplementedError, match="axis 1"):
        check(args, problem, state, axis=1)


def test_refuses_multigrid_field():
    args, problem, state = diffusion("--multigrid", "1")
    with pytest.raises(NotImplementedError, match="MultigridField"):
        check(args, problem, state)


def test_refuses_several_unknowns():
    import darcy

    args = darcy.parse_args(["--ndim", "3", "--N", "8"])
    problem, state = darcy.make_problem(args)
    assert len(state.fields) > 1
    with pytest.raises(NotImplementedError, match="unknowns"):
        check(args, problem, state)


@pytest.mark.parametrize("kind", ["Array", "NeuralNet"])
def test_refuses_parameter_unknowns(kind):
    import odil_amd as odil

    args, problem, _ = diffusion()
    if kind == "Array":
        field = odil.core.Array(array=torch.zeros(3, dtype=torch.float64))
    else:
        field = odil.core.NeuralNet(weights=[torch.zeros(2, 2, dtype=torch.float64)], biases=[torch.zeros(2, dtype=torch.float64)])
    state = odil.State(fields={"u": field}, initialized=True)
    with pytest.raises(NotImplementedError, match=kind):
        check(args, problem, state)


@pytest.mark.parametrize("flag", ["--linsolver_damp", "--linsolver_dampdiag"])
def test_refuses_damping(flag):
    args, problem, state = diffusion(flag, "0.1")
    with pytest.raises(NotImplementedError, match="damping"):
        check(args, problem, state)


@pytest.mark.parametrize("linsolver", ["cg", "bicgstab", "lsqr", "directsq"])
def test_refuses_other_linsolvers(linsolver):
    args, problem, state = diffusion("--linsolver", linsolver)
    with pytest.raises(NotImplementedError, match="linsolver '{}'".format(linsolver)):
        check(args, problem, state)


def test_refuses_uneven_cut():
    args, problem, state = diffusion()
    with pytest.raises(NotImplementedError, match="16 cells on axis 0 over 3 ranks"):
        check(args, problem, state, world=3)


def stencil_problem(reads, nout=1):
    """One cell-centred field on 16^3 with an operator that reads u at `reads` (shifts) and returns `nout` outputs."""
    import odil_amd as odil

    domain = odil.Domain(cshape=[16, 16, 16], dimnames=["x", "y", "z"], dtype=np.float64)

    def operator(ctx):
        res = ctx.field("u")
        for shift in reads:
            res = res + 0.5 * ctx.field("u", *shift) ** 2
        return [res * (k + 1) for k in range(nout)]

    state = odil.State()
    state.fields["u"] = None
    state = domain.init_state(state)
    args = argparse.Namespace(linsolver="multigrid", linsolver_damp=0, linsolver_dampdiag=0)
    return args, odil.Problem(operator, domain, None), state


@pytest.mark.parametrize("reads", [[(2, 0, 0)], [(0, 0, -2)], [(1, 1, 0)], [(-1, 0, 0), (0, 1, -1)]])
def test_refuses_wider_stencils(reads):
    args, problem, state = stencil_problem(reads)
    with pytest.raises(NotImplementedError, match=r"\(2 d \+ 1\)-point"):
        check(args, problem, state)


def test_admits_partial_stencil():
    """A Jacobian with only some of the 2 d + 1 shifts is a (2 d + 1)-point one: the missing shifts are zero arrays."""
    args, problem, state = stencil_problem([(1, 0, 0), (0, 0, -1)])
    assert check(args, problem, state, world=2) is None


def test_refuses_two_outputs():
    args, problem, state = stencil_problem([(1, 0, 0)], nout=2)
    with pytest.raises(NotImplementedError, match="2 outputs"):
        check(args, problem, state)


# ---- the coefficient mapping ---------------------------------------------------------------------------------------------
WANT = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]


def test_mapping_orders_cut_axis_first_and_fills_missing_shifts():
    from odil_amd.gmg import stencil_coefficients

    shape = (4, 6, 8)
    rng = np.random.default_rng(3)
    arrays = {s: torch.tensor(rng.standard_normal(shape)) for s in WANT}
    # the kernel's read order differs from the wanted one; +e_1 does not occur; periodic shifts of the GLOBAL extents
    order = [(0, 0, 1), (1, 0, 0), (0, 0, 0), (0, -1, 0), (0, 0, -1), (-1, 0, 0)]
    period = (12, 6, 8)
    spelled = {(1, 0, 0): (1 - 12, 0, 0), (0, 0, -1): (0, 0, 7)}  # rolls by n - 1 are shifts of -1 and vice versa
    items = [(spelled.get(s, s), arrays[s]) for s in order]
    c = stencil_coefficients(items, shape, period=period)
    assert tuple(c.shape) == (7,) + shape
    for slot, s in enumerate(WANT):
        want = arrays[s] if s != (0, 1, 0) else torch.zeros(shape, dtype=torch.float64)
        assert torch.equal(c[slot], want), (slot, s)


def test_mapping_is_a_view_of_the_kernel_buffer():
    from odil_amd.gmg import stencil_coefficients

    shape = (4, 6, 8)
    buf = torch.arange(8 * 4 * 6 * 8, dtype=torch.float64).view((8,) + shape)
    c = stencil_coefficients([(s, buf[1 + j]) for j, s in enumerate(WANT)], shape, period=(8, 6, 8))
    assert c.data_ptr() == buf[1].data_ptr() and torch.equal(c, buf[1:])


def test_mapping_refuses():
    from odil_amd.gmg import stencil_coefficients

    shape = (4, 6, 8)
    a = torch.ones(shape, dtype=torch.float64)
    assert stencil_coefficients([((0, 0, 0), a), ((0, 2, 0), a)], shape) is None  # not a unit shift
    assert stencil_coefficients([((1, 0, 0), a)], shape) is None  # no centre
