"""The ORDER in which `linsolver.solve` tries its solvers (odil_amd/linsolver.py: ROUTES), on the host: every route of the
table is replaced by a recorder that refuses, so the routes attempted for a request are read off without a device.  The
expected sequences are written out here from the rules the table must keep (reference src/odil/linsolver.py:4-87 has one
solver per `--linsolver` value; the order among this package's solvers is its own contract)."""

import argparse
import itertools

import pytest
import torch

from odil_amd import linsolver as ls
from odil_amd.core import LinearizedOperator

ORDER = ("poisson_cycles", "stencil_cycles", "substitution", "block_cyclic_reduction", "schur_complement",
         "dense_factorisation", "direct_multigrid", "normal_multigrid", "jacobi_cg")
WIDE = ORDER[2:8]  # the routes that see a float64 copy of a float32 problem


def stub_operator(n, dtype, dense):
    """What `solve` and the table's tests read of an operator, and no more."""
    op = object.__new__(LinearizedOperator)
    op.nrows = op.ncols = n
    op.domain, op.dtype, op.device = None, dtype, torch.device("cpu")
    op.blocks = [(0, n, "dense", "w", torch.zeros(1, 1, dtype=dtype))] if dense else []
    return op


def namespace(damp=0.0):
    return argparse.Namespace(linsolver_tol=1e-10, linsolver_maxiter=None, linsolver_damp=damp, linsolver_dampdiag=0)


@pytest.fixture
def recorded(monkeypatch):
    """The table with every route replaced by a recorder of (name, dtype of the operator it was given)."""
    assert tuple(entry[0].__name__ for entry in ls.ROUTES) == ORDER
    seen = []

    def recorder(name):
        def route(req):
            seen.append((name, req.op.dtype))
            return None

        return route

    monkeypatch.setattr(ls, "ROUTES", tuple((recorder(route.__name__), applies, wide) for route, applies, wide in ls.ROUTES))
    # (the memory probe of the dense factorisation asks the device: here, memory permitting)
    monkeypatch.setattr(ls, "_dense_fits", lambda op: op.ncols <= ls.DENSE_MAX_UNKNOWNS)
    return seen


def expected(linsolver, n, damped, dense):
    """The routes attempted when every one refuses, from the table of the routing contract."""
    exact = linsolver in ("direct", "directsq")
    want = []
    if not damped and (linsolver == "multigrid" or (linsolver == "direct" and n > 49152)):
        want += ["poisson_cycles", "stencil_cycles"]
    if not damped and (exact or linsolver == "multigrid"):
        want.append("substitution")
    if exact:
        want.append("block_cyclic_reduction")
        if dense and not (n <= 49152 and n <= 16384):
            want.append("schur_complement")
        if n <= 49152:
            want.append("dense_factorisation")
        if n > 49152:
            want.append("direct_multigrid")
    if linsolver == "multigrid":
        want.append("normal_multigrid")
    return want + ["jacobi_cg"]


GRID = list(itertools.product(("direct", "directsq", "multigrid", "cg", "bicgstab", "lsqr"), (1000, 20000, 60000),
                              (False, True), (torch.float32, torch.float64), (True, False)))


@pytest.mark.parametrize("linsolver,n,damped,dtype,dense", GRID)
def test_routes_attempted(recorded, linsolver, n, damped, dtype, dense):
    op = stub_operator(n, dtype, dense)
    assert ls.solve(op, torch.zeros(n, dtype=dtype), namespace(1e-3 if damped else 0.0), dict(), linsolver) is None
    want = [(name, torch.float64 if name in WIDE else dtype) for name in expected(linsolver, n, damped, dense)]
    assert recorded == want


def test_some_sequences_spelt_out(recorded):
    """(`expected` above restates the rules; these are the sequences themselves.)"""
    def names(linsolver, n, damp=0.0, dense=False):
        del recorded[:]
        ls.solve(stub_operator(n, torch.float64, dense), torch.zeros(n, dtype=torch.float64), namespace(damp), None, linsolver)
        return [name for name, _ in recorded]

    assert names("direct", 1000) == ["substitution", "block_cyclic_reduction", "dense_factorisation", "jacobi_cg"]
    assert names("direct", 20000, dense=True) == ["substitution", "block_cyclic_reduction", "schur_complement",
                                                  "dense_factorisation", "jacobi_cg"]
    assert names("direct", 60000) == ["poisson_cycles", "stencil_cycles", "substitution", "block_cyclic_reduction",
                                      "direct_multigrid", "jacobi_cg"]
    assert names("direct", 60000, damp=1e-3) == ["block_cyclic_reduction", "direct_multigrid", "jacobi_cg"]
    assert names("directsq", 60000) == ["substitution", "block_cyclic_reduction", "direct_multigrid", "jacobi_cg"]
    assert names("multigrid", 1000) == ["poisson_cycles", "stencil_cycles", "substitution", "normal_multigrid", "jacobi_cg"]
    assert names("multigrid", 1000, damp=1e-3) == ["normal_multigrid", "jacobi_cg"]
    assert names("cg", 60000) == ["jacobi_cg"]
    # dense columns in a system small enough for ONE dense factorisation: no Schur complement
    assert names("direct", 1000, dense=True) == ["substitution", "block_cyclic_reduction", "dense_factorisation", "jacobi_cg"]
    assert names("direct", 60000, dense=True) == ["poisson_cycles", "stencil_cycles", "substitution", "block_cyclic_reduction",
                                                  "schur_complement", "direct_multigrid", "jacobi_cg"]


def test_float32_problems_spelt_out(recorded):
    """Which routes see the float64 copy: everything between the cycles on M and the Jacobi CG."""
    f32, f64 = torch.float32, torch.float64
    ls.solve(stub_operator(60000, f32, True), torch.zeros(60000), namespace(), dict(), "direct")
    assert recorded == [("poisson_cycles", f32), ("stencil_cycles", f32), ("substitution", f64), ("block_cyclic_reduction", f64),
                        ("schur_complement", f64), ("direct_multigrid", f64), ("jacobi_cg", f32)]
    del recorded[:]
    ls.solve(stub_operator(1000, f32, False), torch.zeros(1000), namespace(), dict(), "multigrid")
    assert recorded == [("poisson_cycles", f32), ("stencil_cycles", f32), ("substitution", f64), ("normal_multigrid", f64),
                        ("jacobi_cg", f32)]
    del recorded[:]
    ls.solve(stub_operator(1000, f32, False), torch.zeros(1000), namespace(), dict(), "direct")
    assert recorded == [("substitution", f64), ("block_cyclic_reduction", f64), ("dense_factorisation", f64), ("jacobi_cg", f32)]
    del recorded[:]
    ls.solve(stub_operator(1000, f32, False), torch.zeros(1000), namespace(), dict(), "cg")
    assert recorded == [("jacobi_cg", f32)]


def test_the_first_solution_ends_the_walk(recorded, monkeypatch):
    answer = torch.ones(1000, dtype=torch.float64)
    table = list(ls.ROUTES)
    table[3] = (lambda req: answer, table[3][1], table[3][2])  # block cyclic reduction succeeds on the float64 copy
    monkeypatch.setattr(ls, "ROUTES", tuple(table))
    x = ls.solve(stub_operator(1000, torch.float32, False), torch.zeros(1000), namespace(), dict(), "direct")
    assert [name for name, _ in recorded] == ["substitution"]
    assert x.dtype == torch.float32 and bool((x == 1).all())  # (rounded back to the problem's precision)


def test_refused_poisson_cycles_end_in_cg(recorded, monkeypatch):
    """Row 1 is terminal: cycles that stop short hand their iterate to CG on the normal equations, and its result is
    returned -- no later route is tried."""
    class Refusing:
        def solve(self, b, tol, maxiter, status, copy):
            status.update(residual=0.5, bnorm=1.0, niter=maxiter, method="gmg-vcycle", converged=False, stagnated=False)
            return torch.full_like(b, 2.0)

    calls = []

    def cg(op, rhs, **kw):
        calls.append(kw)
        return torch.full_like(rhs, 3.0)

    monkeypatch.setattr(ls.gmg, "recognise_poisson", lambda op: ((4, 4), [1.0, 1.0]))
    monkeypatch.setattr(ls, "poisson_gmg", lambda *a, **kw: Refusing())
    monkeypatch.setattr(ls, "cg_normal", cg)
    monkeypatch.setattr(ls, "printlog", lambda *a: None)
    monkeypatch.setattr(ls, "_dot", lambda a, b: (a * b).sum())
    monkeypatch.delenv("ODIL_GMG", raising=False)
    monkeypatch.delenv("ODIL_GMG_MIXED", raising=False)
    table = list(ls.ROUTES)
    table[0] = (ls.poisson_cycles,) + table[0][1:]
    monkeypatch.setattr(ls, "ROUTES", tuple(table))
    x = ls.solve(stub_operator(16, torch.float64, False), torch.ones(16, dtype=torch.float64), namespace(), dict(), "multigrid")
    assert recorded == [] and bool((x == 3).all())
    assert len(calls) == 1 and calls[0]["tol"] == 1e-10 and bool((calls[0]["x0"] == 2).all())


def test_bad_arguments(recorded):
    with pytest.raises(ValueError, match="Unknown linsolver=qr"):
        ls.solve(stub_operator(10, torch.float64, False), torch.zeros(10), namespace(), dict(), "qr")
    with pytest.raises(TypeError, match="expects the device operator"):
        ls.solve(torch.eye(10), torch.zeros(10), namespace(), dict(), "direct")
    assert recorded == []
