"""L-BFGS-B ensembles as far as they can be checked without a device: the lock-step driver
(`optimizer.lbfgsb_minimize_ensemble`, one `lbfgsb_member` coroutine per member) on a NumPy double of the ensemble backend
against `lbfgsb_minimize` on every member alone -- every iterate `==`; the refusals of `util.optimize_ensemble`; header,
library and `_lib.EXPORTED` carry the new entry points; the launchers refuse malformed arguments with an error text
before anything is launched (every pointer is a dummy)."""

import os
import re
import sys
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest

from test_lbfgs_host_logic import NumpyVectors, rosenbrock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["odil_lbfgs_probe_batch", "odil_lbfgs_dots3_batch", "odil_lbfgs_lincomb_batch", "odil_lbfgs_axpy_batch",
       "odil_lbfgs_pair_batch", "odil_poisson_adjoint_batch"]


# ---------------------------------------------------------------------------------------------- the lock-step driver
class NumpyEnsemble:
    """Test double of optimizer.EnsembleLbfgsVectors: the same `run(plan)` / `read_probes` / `read_products`, immediate
    NumPy arithmetic with the expressions of `NumpyVectors` on member b's rows.  funs[b](x) -> (f, g)."""

    def __init__(self, funs, x0, m):
        self.nb, self.n, self.m, self.funs = len(funs), x0.shape[1], m, funs
        self.v = {name: np.zeros((self.nb, self.n)) for name in "xtrdge"}
        self.v["x"][...] = x0
        self.w = np.zeros((self.nb, 2 * m, self.n))
        self.scal, self.prod = np.zeros((self.nb, 8)), np.zeros((self.nb, 3, 2 * m))
        self.reads, self.evaluations, self.launches = 0, 0, []

    def run(self, plan):
        v = self.v
        for key, who, scalars in plan:
            self.launches.append((key, tuple(who)))
            for b, s in zip(who, scalars):
                kind = key[0]
                if kind == "copy":
                    v[key[1]][b] = v[key[2]][b]
                elif kind == "pair":
                    stp, slot = s
                    v["r"][b] = v["g"][b] - v["r"][b]
                    if stp != 1.0:
                        v["d"][b] = stp * v["d"][b]
                    if slot >= 0:
                        self.w[b, 2 * slot], self.w[b, 2 * slot + 1] = v["d"][b], v["r"][b]
                elif kind == "scale":
                    v["d"][b] = s[0] * v["g"][b]
                elif kind == "lincomb":
                    nphys, c = s
                    v["d"][b] += c @ self.w[b, :2 * nphys]
                elif kind == "probe_direction":
                    self.scal[b, 0:2] = v["d"][b] @ v["d"][b], v["g"][b] @ v["d"][b]
                elif kind == "set_x":
                    v["x"][b] = v["t"][b] + s[0] * v["d"][b]
                elif kind == "probe_eval":
                    g, d = v["g"][b], v[key[1]][b]
                    self.scal[b, 3:6] = g @ d, g @ g, np.max(np.abs(g))
                elif kind == "products":
                    for j, name in enumerate(key[1:]):
                        self.prod[b, j, :2 * s[0]] = self.w[b, :2 * s[0]] @ v[name][b]
                else:
                    assert kind == "eval", key
            if key == ("eval",):  # ALL members, as the device ensemble evaluates them
                self.evaluations += 1
                for b in range(self.nb):
                    self.scal[b, 6], v["e"][b] = self.funs[b](v["x"][b].copy())

    def read_probes(self):
        self.reads += 1
        return self.scal.copy()

    def read_products(self):
        self.reads += 1
        return self.prod.copy()


def quadratic(cond, n, seed):
    rng = np.random.default_rng(seed)
    a = np.geomspace(1.0, cond, n)
    c = rng.standard_normal(n)

    def fun(x):
        return float(0.5 * np.sum(a * (x - c) ** 2)), a * (x - c)

    return fun


N, M, MAXITER, PGTOL = 12, 3, 25, 1e-5


def members():
    """Four seeded members: Rosenbrock from two starts, a well and an ill conditioned quadratic."""
    rng = np.random.default_rng(7)
    funs = [rosenbrock, rosenbrock, quadratic(4.0, N, 1), quadratic(1e4, N, 2)]
    x0 = np.stack([np.linspace(-1.2, 1.0, N), rng.standard_normal(N) * 0.5, rng.standard_normal(N), rng.standard_normal(N)])
    return funs, x0


def single_runs(funs, x0):
    """[(iterates, evaluations made at each iterate's acceptance, result)] of `lbfgsb_minimize` on every member alone."""
    from odil_amd.optimizer import lbfgsb_minimize

    runs = []
    for fun, start in zip(funs, x0):
        xs, evals, count = [], [], [0]

        def counted(x, fun=fun, count=count):
            count[0] += 1
            return fun(x)

        x = start.copy()
        res = lbfgsb_minimize(x, counted, NumpyVectors(N, M), maxiter=MAXITER, m=M, maxls=20, pgtol=PGTOL, factr=0.0,
                              callback=lambda v, xs=xs, evals=evals, count=count: (xs.append(v.copy()), evals.append(count[0])))
        runs.append((xs, evals, res, x))
    return runs


def test_lock_step_driver_reproduces_every_member_alone():
    from odil_amd.optimizer import lbfgsb_minimize_ensemble

    funs, x0 = members()
    runs = single_runs(funs, x0)
    # the single runs themselves show every case the lock-step driver has to get right
    per_iteration = [np.diff([1] + evals) for _, evals, _, _ in runs]  # (1: the evaluation at the start)
    assert any((steps >= 2).any() for steps in per_iteration), "no iteration with two line-search evaluations"
    assert any(res["nit"] > M + 1 for _, _, res, _ in runs), "no wrapped history"
    converged = [res["task"].startswith("CONVERGENCE: NORM") for _, _, res, _ in runs]
    assert any(converged) and not all(converged), [res["task"] for _, _, res, _ in runs]
    first = min(res["funcalls"] for (_, _, res, _), c in zip(runs, converged) if c)
    assert first < max(res["funcalls"] for _, _, res, _ in runs), "the converging member is not the first to finish"
    assert len({res["funcalls"] for _, _, res, _ in runs}) >= 3, "members do not finish in different rounds"

    backend = NumpyEnsemble(funs, x0, M)
    seen = [[] for _ in funs]
    results, info = lbfgsb_minimize_ensemble(backend, len(funs), MAXITER, m=M, maxls=20, pgtol=PGTOL, factr=0.0,
                                             callback=lambda b: seen[b].append(backend.v["x"][b].copy()))
    for b, (xs, _, res, xfinal) in enumerate(runs):
        assert len(seen[b]) == len(xs) == res["nit"], b
        for k, (got, want) in enumerate(zip(seen[b], xs)):
            assert (got == want).all(), (b, k)
        assert (backend.v["x"][b] == xfinal).all(), b
        for key in ("task", "nit", "funcalls", "warnflag", "f"):
            assert results[b][key] == res[key], (b, key, results[b][key], res[key])
    # a round is ONE evaluation of the ensemble: as many as the slowest member needs, and at most two reads each
    assert info.rounds == backend.evaluations == max(res["funcalls"] for _, _, res, _ in runs)
    assert info.host_reads == backend.reads <= 2 * info.rounds + 2
    # every kind of work ran once per flush for all members that asked for it: no launch per member
    assert len(backend.launches) <= 14 * info.rounds + 14


def test_a_round_costs_the_same_work_for_two_and_for_four_members():
    from odil_amd.optimizer import lbfgsb_minimize_ensemble

    counts = []
    for nb in (2, 4):
        funs = [quadratic(50.0, N, 3)] * nb
        x0 = np.stack([np.linspace(-1.0, 1.0, N)] * nb)
        backend = NumpyEnsemble(funs, x0, M)
        _, info = lbfgsb_minimize_ensemble(backend, nb, 6, m=M, maxls=20, pgtol=0.0)
        counts.append((info.rounds, info.host_reads, len(backend.launches)))
    assert counts[0] == counts[1], counts


# ------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture()
def api(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    return odil, poisson


def test_optimize_ensemble_refusals_of_the_lbfgsb_branch(api):
    odil, poisson = api
    base = "--multigrid 1 --ndim 2 --N 16 "
    built = [poisson.make_problem(poisson.parse_args(base.split())) for _ in range(2)]
    problems, states = [p for p, _ in built], [s for _, s in built]

    def args(**kw):
        a = poisson.parse_args(base.split())
        a.epoch_start, a.epochs, a.optimizer = 0, 2, "lbfgsb"
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    run = odil.util.optimize_ensemble
    with pytest.raises(ValueError, match="form 'workgroup' runs whole Adam epochs"):
        run(args(), problems, states)  # (the default form)
    with pytest.raises(ValueError, match="form 'workgroup'"):
        run(args(), problems, states, form="workgroup")
    with pytest.raises(ValueError, match="`lrs` are Adam's"):
        run(args(), problems, states, form="launches", lrs=[1e-2, 1e-3])
    with pytest.raises(ValueError, match="bfgs_m = 65 .*at most 64"):
        run(args(bfgs_m=65), problems, states, form="launches")
    for name in ("gd", "newton", "lbfgs"):
        with pytest.raises(ValueError, match="not optimizer '{}'".format(name)):
            run(args(optimizer=name), problems, states, form="launches")
    with pytest.raises(ValueError, match="is none of"):
        run(args(), problems, states, form="graph")
    # nothing above touched a state
    for (_, fresh), state in zip([poisson.make_problem(poisson.parse_args(base.split())) for _ in range(2)], states):
        for a, b in zip(problems[0].domain.arrays_from_state(fresh), problems[0].domain.arrays_from_state(state)):
            assert (a == b).all()


# ------------------------------------------------------------------------------------------------- the entry points
def test_library_header_and_bindings_carry_the_new_entry_points():
    from odil_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    declared = set(re.findall(r"\b(odil_\w+)\s*\(", header))
    for name in [n + s for n in NEW for s in ("_f64", "_f32")] + ["odil_lbfgs_batch_partials"]:
        assert hasattr(lib, name) and name in _lib.EXPORTED and name in declared, name
    part = lib.odil_lbfgs_batch_partials
    assert part(336, 6, 8) == 3 * 6 * 1 and part(16384, 1, 8) == 3 * 8  # (8 chunks of 256 x 8 for the read-once kernel)
    assert part(16384, 1, 4) == 3 * 8 and part(0, 1, 8) == 0 and part(8, 1, 2) == 0


def _refused(lib, entry, status, text):
    assert status == -1, (entry, text, status)
    err = lib.odil_last_error()
    assert entry.encode() in err and text in err, (entry, text, err)


P = lambda k: c_void_p(4096 * (k + 1))


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_vector_launchers_refuse_before_launching(suffix):
    from odil_amd import _lib

    lib = _lib.load()
    real = (lambda v: v)
    n, nb, rows = 336, 5, 6
    need = lib.odil_lbfgs_batch_partials(n, rows, 8 if suffix == "f64" else 4)

    def probe(g=P(0), d=P(1), gs=n, ds=n, n_=n, nbatch=nb, members=None, nsel=0, part=P(2), ps=need, plen=None, out=P(3), os_=8):
        plen = (nbatch - 1) * ps + need if plen is None else plen
        return getattr(lib, "odil_lbfgs_probe_batch_" + suffix)(g, c_int64(gs), d, c_int64(ds), c_int64(n_), c_int(nbatch), members,
                                                               c_int(nsel), part, c_int64(ps), c_int64(plen), out, c_int64(os_), None)

    refused = lambda text, **kw: _refused(lib, "lbfgs_probe_batch", probe(**kw), text)
    for key in ("g", "d", "part", "out"):
        refused(b"null pointer", **{key: None})
    for nbatch in (0, -1, 65536):
        refused(b"members", nbatch=nbatch)
    refused(b"a list of 6 members for 5", members=P(4), nsel=6)
    refused(b"a list of -1 members", members=P(4), nsel=-1)
    refused(b"below the 336 elements", gs=n - 1)
    refused(b"below the 336 elements", ds=0)
    refused(b"n=0", n_=0)
    refused(b"workspace too short", ps=2)
    refused(b"workspace too short", plen=4 * need + 2)
    assert probe(members=P(4), nsel=0) == 0  # (an empty list: nothing to do, nothing launched)

    def dots3(a=P(0), as_=rows * n, lda=n, rows_=rows, counts=P(1), mc=rows, b0=P(2), s0=n, b1=P(3), s1=n, b2=None, s2=0, n_=n,
              nbatch=nb, members=None, nsel=0, part=P(5), ps=need, plen=None, out=P(6), os_=3 * rows, ldo=rows):
        plen = (nbatch - 1) * ps + need if plen is None else plen
        return getattr(lib, "odil_lbfgs_dots3_batch_" + suffix)(
            a, c_int64(as_), c_int64(lda), c_int(rows_), counts, c_int(mc), b0, c_int64(s0), b1, c_int64(s1), b2, c_int64(s2),
            c_int64(n_), c_int(nbatch), members, c_int(nsel), part, c_int64(ps), c_int64(plen), out, c_int64(os_), c_int64(ldo), None)

    refused = lambda text, **kw: _refused(lib, "lbfgs_dots3_batch", dots3(**kw), text)
    for key in ("a", "b0", "part", "out"):
        refused(b"null pointer", **{key: None})
    for nbatch in (0, 65536):
        refused(b"members", nbatch=nbatch)
    refused(b"count 7 outside 1 ... 6", mc=7)
    refused(b"count 0 outside 1 ... 6", mc=0)
    refused(b"of the history is below", as_=rows * n - 1)
    refused(b"lda=335", lda=n - 1)
    refused(b"of b1 is below", s1=n - 1)
    refused(b"ldo=5", ldo=5)
    refused(b"workspace too short", ps=need - 1)
    # member strides off the 16-byte grid: members would not all run the kernel their single calls run
    item = 8 if suffix == "f64" else 4
    refused(b"would not run the same kernel", s0=n + 16 // item - 1)
    refused(b"would not run the same kernel", as_=rows * n + 1)
    # where n and the alignment admit the read-once kernel, the count decides the single call's kernel beyond 128 vectors
    big = 16384
    refused(b"count 130 above 128", n_=big, lda=big, rows_=130, mc=130, as_=130 * big, s0=big, s1=big, ldo=130, os_=390,
            ps=10 ** 9, plen=10 ** 12)

    def lincomb(y=P(0), ys=n, a=P(1), as_=rows * n, lda=n, rows_=rows, counts=P(2), mc=rows, coef=P(3), cs=rows, n_=n, nbatch=nb):
        return getattr(lib, "odil_lbfgs_lincomb_batch_" + suffix)(y, c_int64(ys), real(1.0), a, c_int64(as_), c_int64(lda), c_int(rows_),
                                                                 counts, c_int(mc), coef, c_int64(cs), c_int64(n_), c_int(nbatch),
                                                                 None, c_int(0), None)

    refused = lambda text, **kw: _refused(lib, "lbfgs_lincomb_batch", lincomb(**kw), text)
    for key in ("y", "a", "coef"):
        refused(b"null pointer", **{key: None})
    refused(b"count 7 outside 0 ... 6", mc=7)
    refused(b"of coef is below", cs=rows - 1)
    refused(b"of y is below", ys=n - 1)
    refused(b"members", nbatch=0)

    def axpy(out=P(0), os_=n, y=P(1), ys=n, x=P(2), xs=n, alpha=P(3), n_=n, nbatch=nb):
        return getattr(lib, "odil_lbfgs_axpy_batch_" + suffix)(out, c_int64(os_), y, c_int64(ys), x, c_int64(xs), alpha, c_int64(n_),
                                                              c_int(nbatch), None, c_int(0), None)

    refused = lambda text, **kw: _refused(lib, "lbfgs_axpy_batch", axpy(**kw), text)
    refused(b"null pointer", out=None)
    refused(b"null pointer", x=None)
    refused(b"null pointer", alpha=None)  # (y + alpha x needs its alpha)
    refused(b"of out is below", os_=n - 1)
    refused(b"members", nbatch=65536)

    def pair(g=P(0), r=P(1), d=P(2), w=P(3), ws=rows * n, lda=n, rows_=rows, stp=P(4), slot=P(5), gs=n, nbatch=nb):
        return getattr(lib, "odil_lbfgs_pair_batch_" + suffix)(g, c_int64(gs), r, c_int64(n), d, c_int64(n), w, c_int64(ws), c_int64(lda),
                                                              c_int(rows_), stp, slot, c_int64(n), c_int(nbatch), None, c_int(0), None)

    refused = lambda text, **kw: _refused(lib, "lbfgs_pair_batch", pair(**kw), text)
    for key in ("g", "r", "d", "w", "stp", "slot"):
        refused(b"null pointer", **{key: None})
    refused(b"an even number", rows_=5)
    refused(b"of the history is below", ws=rows * n - 1)
    refused(b"of g is below", gs=1)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_adjoint_launcher_refuses_before_launching(suffix):
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_poisson_adjoint_batch_" + suffix)
    h2 = np.array([0.25, 0.5, 1.0], dtype=np.float64 if suffix == "f64" else np.float32)

    def launch(fu=P(0), gu=P(1), nbatch=3, fs=128, gs=128, shp=(16, 8), ndim=2, h=True):
        return fn(fu, gu, c_int(nbatch), c_int64(fs), c_int64(gs), _lib.i64(shp) if shp else None, c_int(ndim),
                  h2.ctypes.data_as(c_void_p) if h else None, 1.0, None)

    refused = lambda text, **kw: _refused(lib, "poisson_adjoint_batch", launch(**kw), text)
    refused(b"null pointer", fu=None)
    refused(b"null pointer", gu=None)
    refused(b"null pointer", shp=None)
    refused(b"null pointer", h=False)
    for nbatch in (0, 65536):
        refused(b"members", nbatch=nbatch)
    refused(b"ndim 4", ndim=4, shp=(4, 4, 4, 4))
    refused(b"ndim 0", ndim=0)
    refused(b"smaller than a member", fs=127)
    refused(b"not a multiple of 16 bytes", gs=129)
    refused(b"smaller than a member", ndim=3, shp=(8, 8, 8), fs=511, gs=512)
