"""The hand-over to GCR inside the one-launch Newton solve of an ensemble, without a device: the new entry points in
header, library and binding, their work size, what the launcher refuses before any launch, the refusals of
`util.optimize_newton_ensemble(krylov=...)`, and -- in the NumPy model tests/ensemble_krylov_np.py -- the facts the cases
of tests/test_newton_ensemble_krylov_gpu.py rest on."""

import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch
from conftest import ROOT

import ensemble_krylov_np as model
import stencil_gmg_np as sg

NAMES = ("odil_stencil_solve_krylov_batch_f64", "odil_stencil_solve_krylov_batch_f32",
         "odil_stencil_solve_krylov_batch_work")
LEVELS = {(64,): [(64,), (32,), (16,), (8,), (4,), (2,)], (16, 16): [(16, 16), (8, 8), (4, 4), (2, 2)],
          (8, 8, 8): [(8, 8, 8), (4, 4, 4), (4, 2, 2)]}


def test_the_new_entry_points_are_declared_built_and_bound():
    from odil_amd import _lib

    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + "(" in header and name in _lib.EXPORTED and hasattr(lib, name), name
    f64 = lib.odil_stencil_solve_krylov_batch_f64
    assert len(f64.argtypes) == len(lib.odil_stencil_solve_batch_f64.argtypes) + 1 and f64.argtypes[-2] is ctypes.c_int


def flat(shapes):
    return (ctypes.c_int64 * sum(len(s) for s in shapes))(*[n for s in shapes for n in s])


@pytest.mark.parametrize("shape", sorted(LEVELS), ids=["16x16", "64", "8^3"])
def test_the_work_size_adds_the_vectors_of_gcr(shape):
    from odil_amd import _lib, ops

    lib, shapes = _lib.load(), LEVELS[shape]
    old = lib.odil_stencil_solve_batch_work(flat(shapes), len(shapes), len(shape))
    assert old == 3 * sum(math.prod(s) for s in shapes)
    for m in (1, 6, 8):
        new = lib.odil_stencil_solve_krylov_batch_work(flat(shapes), len(shapes), len(shape), m)
        assert new == old + (2 * m + 2) * math.prod(shape) == ops.stencil_solve_krylov_batch_work(shapes, m)
    for m in (0, 9, -1):
        assert lib.odil_stencil_solve_krylov_batch_work(flat(shapes), len(shapes), len(shape), m) == 0


def test_the_work_size_of_malformed_shapes_is_zero():
    from odil_amd import _lib

    work = _lib.load().odil_stencil_solve_krylov_batch_work
    assert work(None, 1, 1, 6) == 0 and work(flat([(8,)]), 0, 1, 6) == 0 and work(flat([(8,)]), 1, 4, 6) == 0
    assert work(flat([(0,)]), 1, 1, 6) == 0 and work(flat([(65536,)]), 1, 1, 6) == 0
    assert work(flat([(8,)] * 9), 9, 1, 6) == 0 and work(flat([(2048, 1024)]), 1, 2, 6) == 0


def refusal(dtype=np.float64, **change):
    """(status, error text) of the launcher for a well-formed call with `change` applied; no pointer is ever followed."""
    from odil_amd import _lib

    lib = _lib.load()
    real = ctypes.c_double if dtype == np.float64 else ctypes.c_float
    shapes = [(8,), (4,)]
    need = 3 * 12 + 14 * 8
    buf = (real * 1024)()
    hist = (ctypes.c_double * 64)()
    out = (ctypes.c_int * 6)()
    w = (real * 2)(0.8, 0.8)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    halve = (ctypes.c_int * 1)(1)
    kw = dict(coeffs=p(buf), coeff_stride=0, shapes=flat(shapes), halve=p(halve), nlev=2, ndim=1, nbatch=2, x=p(buf), x_stride=8,
              b=ctypes.c_void_p(ctypes.addressof(buf) + 512), b_stride=8, work=p(buf), work_stride=need, work_len=2 * need,
              inv=p(buf), inv_stride=0, ninv=4, wpre=p(w), npre=2, wpost=p(w), npost=2, start=2, mode=0, maxcycles=20, tol=1e-10,
              history=p(hist), history_stride=22, outcome=p(out), krylov_m=6, stream=None)
    kw.update(change)
    fn = lib.odil_stencil_solve_krylov_batch_f64 if dtype == np.float64 else lib.odil_stencil_solve_krylov_batch_f32
    return fn(*kw.values()), lib.odil_last_error()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_launcher_refuses_before_any_launch(dtype):
    need = 3 * 12 + 14 * 8
    for change, text in ((dict(krylov_m=0), b"krylov_m 0"), (dict(krylov_m=9), b"krylov_m 9"),
                         (dict(work_len=2 * need - 1), b"work array"), (dict(work_stride=need - 1), b"stride smaller"),
                         (dict(outcome=None), b"null pointer"), (dict(mode=1, start=1), b"a Newton step starts from"),
                         (dict(maxcycles=1001), b"maxcycles"), (dict(history_stride=21), b"history_stride")):
        status, err = refusal(dtype, **change)
        assert status != 0 and b"stencil_solve_krylov_batch" in err and text in err, (change, err)
    # (the old work size is too small for the new entry: the (2 m + 2) vectors are part of the check)
    status, err = refusal(dtype, work_stride=36, work_len=72)
    assert status != 0 and b"36" in err


# ------------------------------------------------------------------------------------------------------- the driver
N, NB = 8, 3


class UnprobedProblem:
    """A member whose operator must not be looked at: every refusal below comes first."""

    def __init__(self, domain):
        self.domain = domain

    def __getattr__(self, name):
        raise AssertionError("the member was probed ({})".format(name))


@pytest.fixture
def members(monkeypatch):
    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    domains = [odil.Domain(cshape=[N], multigrid=False, dtype=np.float64) for _ in range(NB)]
    problems = [UnprobedProblem(domain) for domain in domains]
    return odil, problems, [domain.init_state(odil.State(fields={"u": None})) for domain in domains]


def test_the_driver_refuses_other_values_and_the_batched_launches(members):
    odil, problems, states = members
    args = argparse.Namespace(epoch_start=0, epochs=1, linsolver="multigrid", linsolver_tol=1e-10)
    with pytest.raises(ValueError, match="krylov 'sometimes' is neither 'never' nor 'auto'"):
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="sometimes")
    with pytest.raises(ValueError, match="krylov 'auto' with form 'launches'"):
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="auto", form="launches")


def test_form_auto_names_the_member_that_needs_the_batched_launches(monkeypatch):
    """Member 1 is beyond one workgroup: form 'auto' would run everything as batched launches, which have no hand-over --
    the option is not dropped, the member and the reason are named, and no operator is probed."""
    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    domains = [odil.Domain(cshape=[65536], multigrid=False, dtype=np.float64) for _ in range(NB)]
    problems = [UnprobedProblem(domain) for domain in domains]
    states = [domain.init_state(odil.State(fields={"u": None})) for domain in domains]
    args = argparse.Namespace(epoch_start=0, epochs=1, linsolver="multigrid", linsolver_tol=1e-10)
    with pytest.raises(ValueError, match=r"member 0.*65536 cells.*no hand-over to GCR \(krylov 'auto'\)"):
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="auto", form="auto")
    with pytest.raises(ValueError, match="member 0.*65536 cells"):  # (form 'workgroup': its own refusal, as before)
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="auto")


def test_the_extra_work_memory_is_checked_against_the_free_memory(monkeypatch):
    from odil_amd import ensemble

    need = 64 * 14 * 32 ** 3 * 8
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (need - 1, 1 << 40))
    reason = ensemble._krylov_memory_refusal(64, (32, 32, 32), torch.float64, torch.device("cuda:0"), 6)
    assert reason is not None and "{} bytes of work memory".format(need) in reason and "{} bytes of device".format(need - 1) in reason
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (need, 1 << 40))
    assert ensemble._krylov_memory_refusal(64, (32, 32, 32), torch.float64, torch.device("cuda:0"), 6) is None
    assert ensemble._krylov_memory_refusal(64, (32, 32, 32), torch.float32, torch.device("cpu"), 6) is None


def test_the_solver_classes_take_or_refuse_the_keyword():
    from odil_amd import gmg

    assert "krylov" in gmg.EnsembleGMG.core and gmg.EnsembleGMG.krylov == "never" and gmg.EnsembleGMG.krylov_m == 6
    coeffs = torch.zeros((2, 3, 8), dtype=torch.float64)
    with pytest.raises(ValueError, match="neither 'never' nor 'auto'"):
        gmg.EnsembleGMG.from_coeffs(coeffs, krylov="always")
    with pytest.raises(ValueError, match="krylov_m = 9"):
        gmg.EnsembleGMG.from_coeffs(coeffs, krylov="auto", krylov_m=9)
    with pytest.raises(ValueError, match="EnsembleLaunchGMG: krylov 'auto'"):
        gmg.EnsembleLaunchGMG.from_coeffs(coeffs, krylov="auto")


def test_status_reports_the_hand_over_and_the_breakdown():
    from odil_amd import gmg

    ens = gmg.EnsembleGMG.__new__(gmg.EnsembleGMG)
    ens.method, ens.cells, ens.krylov_m = "stub", 4, 6
    ens.history = np.array([[4.0, 1.0, 0.25, 1e-24, 0.0], [4.0, 1.0, 0.5, 0.4, 0.3], [4.0, 1.0, 0.5, 0.0, 0.0]])
    ens.outcome = np.array([[2, 0, -1], [3, 0, 2], [1, 4, 1]], dtype=np.int32)
    plain, handed, broken = (ens.status(m) for m in range(3))
    assert plain["handover"] is None and plain["method"] == "stub" and plain["converged"] and plain["niter"] == 2
    assert handed["handover"] == 2 and handed["method"] == "stub + GCR(6)" and handed["niter"] == 3
    assert broken["handover"] == 1 and not broken["converged"] and not broken["stagnated"]


# -------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def modelled():
    """Per case and member: (levels, the solve with krylov="never", with "auto") at the case's budget -- computed once."""
    out = dict()
    for case in model.CASES:
        name, shape, budget, members, hard, benign = case
        coeffs, b = model.case_arrays(case)
        out[name] = [(model.level_shapes(list(c)), model.solve(list(c), rhs, maxcycles=budget, krylov="never"),
                      model.solve(list(c), rhs, maxcycles=budget, krylov="auto")) for c, rhs in zip(coeffs, b)]
    return out


@pytest.mark.parametrize("case", model.CASES, ids=["A-1d-64", "B-8^3"])
def test_the_model_holds_the_facts_of_the_gpu_cases(modelled, case):
    name, shape, budget, members, hard, benign = case
    runs = modelled[name]
    coeffs, b = model.case_arrays(case)
    assert all(levels == runs[0][0] for levels, _, _ in runs), [levels for levels, _, _ in runs]
    for m, (levels, never, auto) in enumerate(runs):
        print(name, m, members[m][0], levels, "never", never["niter"], never["why"], "auto", auto["niter"], auto["why"],
              auto["handover"])
        assert auto["why"] == model.CONVERGED and auto["niter"] <= budget
        assert np.linalg.norm(sg.apply(list(coeffs[m]), auto["x"]) - b[m]) <= 1e-10 * np.linalg.norm(b[m])
    for m in hard:
        never, auto = runs[m][1:]
        assert never["why"] != model.CONVERGED          # plain cycles do not reach 1e-10 within the budget
        assert auto["handover"] is not None and auto["handover"] >= 2
    for m in benign:
        never, auto = runs[m][1:]
        assert auto["handover"] is None and never["why"] == model.CONVERGED
        assert auto["niter"] == never["niter"] and np.array_equal(auto["x"], never["x"])
    if name == "A":  # (the restart: more passes than directions kept)
        assert runs[1][2]["niter"] - runs[1][2]["handover"] > 6


@pytest.mark.parametrize("shape", [(64,), (16, 16), (8, 8, 8)], ids=["64", "16x16", "8^3"])
def test_the_benign_random_members_never_meet_the_rule(shape):
    coeffs = model.benign_members(shape, 3)
    rng = np.random.default_rng(11)
    levels = [model.level_shapes(list(c)) for c in coeffs]
    assert all(l == levels[0] for l in levels)
    for c in coeffs:
        run = model.solve(list(c), sg.apply(list(c), rng.standard_normal(shape)), krylov="auto")
        assert run["why"] == model.CONVERGED and run["handover"] is None, (shape, run["niter"], run["why"])
