"""Newton systems with more than 63 `Array` / `NeuralNet` parameters: the wide X^T Y kernel (odil_dense_block_xty_wide,
64-column panels of v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 tiles) against NumPy float64, and the Schur
route of `linsolver` that it opens for up to DENSE_COLUMNS_MAX = 1023 dense columns, against host solves of the
assembled normal equations and against the dense factorisation.  Every figure that is asserted on is printed first
(-s)."""

import importlib
import io
import os
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT

import odil_amd as odil
from odil_amd import linsolver, ops

pytestmark = pytest.mark.gpu

NCOEF = 100
EPS = 0.05  # u + EPS * (sum of the four neighbours - 4 u): diagonal 0.8 against 0.2 off it


def to(x, dev):
    return torch.tensor(np.ascontiguousarray(x), device=dev)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_xty_on_the_matrix_cores(dtype):
    """ops.dense_xty beyond 64 columns per operand: row counts that are multiples of nothing, one to sixteen panels
    per operand, a last panel of one column, the Gram call (mirrored below the diagonal: exactly symmetric), column
    slices of a wider matrix; bit-reproducible; the bound of test_dense_block_xty_on_the_matrix_cores."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    tol = 1e-13 if dtype == np.float64 else 2e-5

    def check(got, want, n, what):
        assert got.shape == want.shape, what
        err = np.max(np.abs(got.cpu().numpy() - want))
        bound = tol * max(1.0, np.max(np.abs(want))) * np.sqrt(n)
        print("dense_xty", np.dtype(dtype).name, what, "error", err, "bound", bound)
        assert err <= bound, what

    for n, px, py in [(5, 65, 1), (257, 64, 65), (4099, 65, 65), (3001, 141, 142), (100003, 97, 98), (70001, 200, 1),
                      (1000, 1024, 1024), (2049, 1, 1000)]:
        x, y = rng.standard_normal((n, px)).astype(dtype), rng.standard_normal((n, py)).astype(dtype)
        tx, ty = to(x, dev), to(y, dev)
        got = ops.dense_xty(tx, ty)
        check(got, x.astype(np.float64).T @ y.astype(np.float64), n, (n, px, py))
        assert torch.equal(got, ops.dense_xty(tx, ty)), (n, px, py)
    # the Gram call: X and Y are the same matrix
    d = rng.standard_normal((3001, 130)).astype(dtype)
    td = to(d, dev)
    got = ops.dense_xty(td, td)
    check(got, d.astype(np.float64).T @ d.astype(np.float64), 3001, "gram 130")
    assert torch.equal(got, got.t())
    assert torch.equal(got, ops.dense_xty(td, td))
    # column slices of one wider matrix (row stride > columns): [D | r] as the solver passes it
    d = rng.standard_normal((3001, 142)).astype(dtype)
    td = to(d, dev)
    got = ops.dense_xty(td[:, :141], td)
    check(got, d[:, :141].astype(np.float64).T @ d.astype(np.float64), 3001, "slices 141 / 142")
    assert torch.equal(got[:, :141], got[:, :141].t())
    assert torch.equal(got, ops.dense_xty(td[:, :141], td))
    # ... and against a copy of the slice, which does not take the mirrored path: the same numbers to the bound
    check(ops.dense_xty(td[:, :141].contiguous(), td), d[:, :141].astype(np.float64).T @ d.astype(np.float64), 3001,
          "copy 141 / 142")
    with pytest.raises(ValueError, match="1024"):
        ops.dense_xty(torch.zeros((8, 1025), dtype=td.dtype, device=dev), td[:8])
    with pytest.raises(ValueError, match="1024"):
        ops.dense_xty(td[:8], torch.zeros((8, 1025), dtype=td.dtype, device=dev))


def basis_operator(ctx):
    """u + EPS laplace(u) + sum_k a[k] phi_k - f on a periodic grid, and the coefficients themselves (without that
    output M = [S | Phi] has more columns than rows)."""
    extra = ctx.extra
    u = ctx.field("u")
    lap = ctx.field("u", -1, 0) + ctx.field("u", 1, 0) + ctx.field("u", 0, -1) + ctx.field("u", 0, 1) - u * 4
    a = ctx.field("a")
    fit = (a[:, None, None] * extra.phi).sum(dim=0)
    return [("fu", u + lap * EPS + fit - extra.f), ("areg", a * extra.areg)]


def basis_system(nx, ny):
    """(op, rhs) of `basis_operator` through the public API; phi_k: unit-variance noise over sqrt(cells), so that the
    columns of Phi have norms near one at every grid size."""
    import argparse

    mod = odil.runtime.get_mod()
    rng = np.random.default_rng(11)
    domain = odil.Domain(cshape=(nx, ny), dimnames=["x", "y"], lower=(0, 0), upper=(1, 1), dtype=np.float64,
                         multigrid=0)
    state = odil.State(fields={
        "u": odil.Field(rng.standard_normal((nx, ny)), loc="cc"),
        "a": odil.Array(rng.standard_normal(NCOEF)),
    })
    state = domain.init_state(state)
    extra = argparse.Namespace(phi=mod.array(rng.standard_normal((NCOEF, nx, ny)) / np.sqrt(nx * ny)),
                               f=mod.array(rng.standard_normal((nx, ny))), areg=0.5)
    problem = odil.Problem(basis_operator, domain, extra)
    vector, op = problem.linearize_device(state)
    return op, vector.contiguous()


def damped_host(m, y, damp, dampdiag):
    a = m.T @ m
    a = a + damp ** 2 * np.eye(len(a))  # reference linsolver.py:19-23: damp first, dampdiag on the damped diagonal
    return np.linalg.solve(a + dampdiag ** 2 * np.diag(np.diag(a)), m.T @ y)


def rel(a, b):
    a = a.detach().cpu().numpy()
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))


def normal_residual(op, x, rhs):
    """|M^T (M x - rhs)| / |M^T rhs|"""
    return float((op.rmatvec(op.matvec(x) - rhs)).norm()) / float(op.rmatvec(rhs).norm())


def test_schur_route_with_100_coefficients_vs_host_solve():
    op, rhs = basis_system(48, 40)
    assert op.shape == (48 * 40 + NCOEF, 48 * 40 + NCOEF)
    m = op.to_dense().cpu().numpy()
    y = rhs.cpu().numpy()
    st = dict()
    x = linsolver.schur_normal(op, rhs, status=st)
    assert x is not None
    assert st["method"] == "schur-mfma" and st["dense_columns"] == NCOEF
    err = rel(x, np.linalg.solve(m.T @ m, m.T @ y))
    print("schur, 100 columns: error", err, "status", st)
    assert err < 1e-9
    x = linsolver.schur_normal(op, rhs, damp=0.3, dampdiag=0.2)
    err = rel(x, damped_host(m, y, 0.3, 0.2))
    print("schur, 100 columns, damped: error", err)
    assert err < 1e-9


def test_direct_beyond_the_dense_factorisation_takes_the_schur_route():
    import argparse

    small, rhs_small = basis_system(48, 40)
    yardstick = normal_residual(small, linsolver.dense_normal(small, rhs_small), rhs_small)
    op, rhs = basis_system(256, 256)
    assert op.ncols == 65536 + NCOEF > linsolver.DENSE_MAX_UNKNOWNS
    st = dict()
    args = argparse.Namespace(linsolver_damp=0, linsolver_dampdiag=0, linsolver_tol=1e-10, linsolver_maxiter=None)
    x = linsolver.solve(op, rhs, args, st, "direct")
    assert st["method"].startswith("schur-mfma"), st
    assert st["dense_columns"] == NCOEF
    assert np.isfinite(st["inner_residual_max"])
    res = normal_residual(op, x, rhs)
    print("direct, 256 x 256 + 100: residual", res, "dense_normal on 48 x 40:", yardstick, "status", st)
    # (ten times the yardstick for the longer reductions at 34 times the rows per column)
    # measured on an MI355X: 1.2e-15 here, 7.7e-16 for dense_normal on 48 x 40 -- the 1e-10 floor decides
    assert res <= max(10 * yardstick, 1e-10)


def heat_system(argv):
    p = os.path.join(ROOT, "examples", "heat")
    if p not in sys.path:
        sys.path.insert(0, p)
    heat = importlib.import_module("heat")
    odil.util.set_log_file(open(os.devnull, "w"))
    args = heat.parse_args(argv + ["--multigrid", "0", "--double", "1"])
    problem, state = heat.make_problem(args)
    vector, op = problem.linearize_device(state)
    return op, vector.contiguous()


def test_heat_with_97_weights_through_block_cyclic_reduction():
    """examples/heat with --arch_k 8 8 (8 + 8 + 64 + 8 + 8 + 1 weights): the block-tridiagonal inner solver under the
    Schur complement.  The weights leave the complement singular and the routes pick different members of the solution
    set: the residuals of the normal equations are compared, the dense factorisation is the yardstick."""
    np.random.seed(1)
    odil.runtime.get_mod().random.set_seed(1)
    op, rhs = heat_system(["--Nt", "32", "--Nx", "32", "--infer_k", "1", "--arch_k", "8", "8"])
    st = dict()
    x = linsolver.blocktri_normal(op, rhs, status=st)
    assert x is not None
    assert "block-tridiagonal" in st["method"] and st["dense_columns"] == 97, st
    assert bool(torch.isfinite(x).all())
    dense = linsolver.dense_normal(op, rhs)
    assert dense is not None
    res, yardstick = normal_residual(op, x, rhs), normal_residual(op, dense, rhs)
    print("heat 32 x 32, 97 weights: schur residual", res, "dense_normal", yardstick, "status", st)
    # measured on an MI355X: Schur route 3.2e-14, dense_normal 2.2e-14 (default weights, no --kwreg: its Cholesky holds)
    # -- the 1e-10 floor decides
    assert res <= max(10 * yardstick, 1e-10)


def test_schur_route_declines_when_memory_is_short(monkeypatch):
    op, rhs = basis_system(48, 40)
    log = io.StringIO()
    monkeypatch.setattr(odil.util, "g_log_file", log)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 288 << 30))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    assert linsolver.schur_normal(op, rhs, status=dict()) is None
    after = torch.cuda.max_memory_allocated()
    assert after - before < op.nrows * (NCOEF + 1) * 8  # [D | r] was never allocated
    lines = [line for line in log.getvalue().splitlines() if "Schur" in line]
    assert len(lines) == 1, log.getvalue()
    need = 6 * op.nrows * (NCOEF + 1) * 8
    assert "{} dense columns".format(NCOEF) in lines[0] and str(need) in lines[0] and str(1 << 20) in lines[0], lines[0]
