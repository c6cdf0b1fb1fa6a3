"""The hand-over to GCR across the batched launches of a Newton ensemble (gmg.EnsembleLaunchKrylovGMG,
`util.optimize_newton_ensemble(krylov="any")`, odil_stencil_gcr_*_batch), what needs no device: the new entry points in
header, library and binding, what they refuse before any launch (ODIL_E_INVAL; the pointers are dummies that are never
followed), the driver's handling of the new value, and -- in the NumPy model tests/ensemble_krylov_np.py -- the level shapes
and splits the cases of tests/test_newton_ensemble_launch_krylov_gpu.py rest on."""

import argparse
import ctypes
import os
from ctypes import c_double, c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch
from conftest import ROOT

import ensemble_krylov_np as model

VECTOR = ("dots", "project", "update", "sumsq")
NAMES = ["odil_stencil_gcr_{}_batch_{}".format(v, s) for v in VECTOR for s in ("f64", "f32")] + [
    "odil_stencil_gcr_decide_batch", "odil_stencil_gcr_batch_parts"]


def test_the_new_entry_points_are_declared_built_and_bound():
    from odil_amd import _lib

    header = open(os.path.join(ROOT, "include", "odil_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + "(" in header and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.odil_stencil_gcr_decide_batch.argtypes[0] is ctypes.c_int
    assert lib.odil_stencil_gcr_decide_batch.argtypes[-1] is ctypes.c_void_p
    makefile = open(os.path.join(ROOT, "odil_amd", "csrc", "Makefile")).read()
    assert "ensemble_gcr.hip" in makefile


def test_the_partial_sums_depend_on_the_cells_alone():
    from odil_amd import _lib, ops

    parts = _lib.load().odil_stencil_gcr_batch_parts
    assert [parts(n) for n in (1, 64, 1024, 1025, 40960, 1 << 24)] == [1, 1, 1, 2, 40, 1 << 14]
    assert parts(0) == 0 and parts(-3) == 0 and parts((1 << 24) + 1) == 0
    assert ops.stencil_gcr_batch_parts(512) == 1


P = dict(store=4096, rho=8192, x=12288, v=16384, have=20480, mask=24576, scal=28672, gpart=32768, history=36864,
         outcome=40960, counts=45056, partials=49152, flags=53248)
CELLS, M, NB = 2048, 6, 3  # (two workgroups per member)
PARTS = 2


def vector_call(which, suffix, **change):
    """(status, error text) of one vector pass for a well-formed call with `change` applied."""
    from odil_amd import _lib

    lib = _lib.load()
    p = {k: c_void_p(v) for k, v in P.items()}
    store = dict(store=p["store"], store_stride=c_int64(2 * M * CELLS))
    common = dict(cells=c_int64(CELLS), krylov_m=c_int(M), slot=c_int(2))
    tail = dict(mask=p["mask"], nbatch=c_int(NB), gpart=p["gpart"], gpart_stride=c_int64((M + 2) * PARTS), stream=None)
    have = dict(have=p["have"], max_have=c_int(M))
    scal = dict(scal=p["scal"], scal_stride=c_int64(M + 2))
    rho = dict(rho=p["rho"], rho_stride=c_int64(CELLS))
    if which == "dots":
        kw = {**store, **common, **have, **tail}
    elif which == "project":
        kw = {**store, **rho, **common, **have, **scal, **tail}
    elif which == "update":
        kw = {**store, "x": p["x"], "x_stride": c_int64(CELLS), **rho, **common, **scal, **tail}
    else:
        kw = {"v": p["v"], "v_stride": c_int64(CELLS), "cells": c_int64(CELLS), **tail}
    for key, value in change.items():
        assert key in kw, (which, key)
        kw[key] = value
    status = getattr(lib, "odil_stencil_gcr_{}_batch_{}".format(which, suffix))(*kw.values())
    return status, lib.odil_last_error()


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_the_vector_passes_refuse_before_any_launch(suffix):
    cases = {
        "dots": [(dict(krylov_m=0), b"krylov_m 0"), (dict(krylov_m=9), b"krylov_m 9"), (dict(nbatch=0), b"nbatch 0"),
                 (dict(nbatch=65536), b"nbatch 65536"), (dict(store_stride=2 * M * CELLS - 1), b"store_stride"),
                 (dict(mask=None), b"mask is null"), (dict(have=None), b"have is null"), (dict(max_have=M + 1), b"beyond krylov_m"),
                 (dict(max_have=-1), b"beyond krylov_m"), (dict(slot=M), b"slot 6"), (dict(slot=-1), b"slot -1"),
                 (dict(gpart_stride=(M + 2) * PARTS - 1), b"gpart_stride"), (dict(gpart=None), b"gpart is null"),
                 (dict(store=None), b"store is null"), (dict(cells=0), b"cells 0"), (dict(cells=(1 << 24) + 1), b"cells")],
        "project": [(dict(krylov_m=9), b"krylov_m 9"), (dict(nbatch=70000), b"nbatch 70000"),
                    (dict(rho_stride=CELLS - 1), b"rho_stride"), (dict(rho=None), b"rho is null"),
                    (dict(scal_stride=M + 1), b"scal_stride"), (dict(scal=None), b"scal is null"),
                    (dict(mask=None), b"mask is null"), (dict(have=None), b"have is null"),
                    (dict(max_have=M + 1), b"beyond krylov_m"), (dict(store_stride=CELLS), b"store_stride")],
        "update": [(dict(krylov_m=0), b"krylov_m 0"), (dict(nbatch=-1), b"nbatch -1"), (dict(x_stride=CELLS - 1), b"x_stride"),
                   (dict(rho_stride=1), b"rho_stride"), (dict(x=None), b"x is null"), (dict(mask=None), b"mask is null"),
                   (dict(scal_stride=0), b"scal_stride"), (dict(x=c_void_p(P["rho"])), b"one array"),
                   (dict(gpart_stride=1), b"gpart_stride")],
        "sumsq": [(dict(nbatch=0), b"nbatch 0"), (dict(v_stride=CELLS - 1), b"v_stride"), (dict(v=None), b"v is null"),
                  (dict(mask=None), b"mask is null"), (dict(gpart_stride=PARTS - 1), b"gpart_stride"), (dict(cells=-5), b"cells -5")],
    }
    for which, changes in cases.items():
        for change, text in changes:
            status, err = vector_call(which, suffix, **{k: (v if v is None or isinstance(v, c_void_p) else
                                                           (c_int64(v) if k.endswith("stride") or k == "cells" else c_int(v)))
                                                        for k, v in change.items()})
            assert status != 0 and b"stencil_gcr_" + which.encode() + b"_batch" in err and text in err, (which, change, err)


def decide_call(**change):
    from odil_amd import _lib

    lib = _lib.load()
    p = {k: c_void_p(v) for k, v in P.items()}
    flag = lambda i: c_void_p(P["flags"] + 64 * i)
    kw = dict(mode=c_int(0), partials=p["partials"], partials_stride=c_int64(8), partials0=None, partials0_stride=c_int64(8),
              nparts=c_int(8), gpart=p["gpart"], gpart_stride=c_int64((M + 2) * PARTS), gparts=c_int(PARTS), nbatch=c_int(NB),
              cells=c_int64(CELLS), k=c_int(2), maxcycles=c_int(20), tol=c_double(1e-10), krylov_m=c_int(M),
              history=p["history"], history_stride=c_int64(22), outcome=p["outcome"], active=flag(0), gcr=flag(1),
              fresh=flag(2), verify=flag(3), have=flag(4), scal=p["scal"], scal_stride=c_int64(M + 2), counts=p["counts"],
              stream=None)
    for key, value in change.items():
        assert key in kw, key
        kw[key] = value
    return lib.odil_stencil_gcr_decide_batch(*kw.values()), lib.odil_last_error()


def test_the_decision_refuses_before_any_launch():
    for change, text in ((dict(mode=c_int(4)), b"mode 4"), (dict(mode=c_int(-1)), b"mode -1"), (dict(krylov_m=c_int(0)), b"krylov_m 0"),
                         (dict(krylov_m=c_int(9)), b"krylov_m 9"), (dict(nbatch=c_int(0)), b"nbatch 0"),
                         (dict(nbatch=c_int(65536)), b"nbatch 65536"), (dict(gcr=None), b"a mask is null"),
                         (dict(active=None), b"a mask is null"), (dict(fresh=None), b"a mask is null"),
                         (dict(verify=None), b"a mask is null"), (dict(have=None), b"a mask is null"),
                         (dict(partials=None), b"null pointer"), (dict(counts=None), b"null pointer"),
                         (dict(outcome=None), b"null pointer"), (dict(history=None), b"null pointer"),
                         (dict(partials_stride=c_int64(7)), b"partials_stride"), (dict(gpart_stride=c_int64((M + 2) * PARTS - 1)), b"gpart_stride"),
                         (dict(scal_stride=c_int64(M + 1)), b"scal_stride"), (dict(history_stride=c_int64(21)), b"history_stride"),
                         (dict(k=c_int(21)), b"pass 21 of at most 20"), (dict(tol=c_double(-1.0)), b"tolerance"),
                         (dict(cells=c_int64(0)), b"cells 0"), (dict(gparts=c_int(0)), b"gparts 0"),
                         (dict(gparts=c_int(65537)), b"gparts 65537")):
        status, err = decide_call(**change)
        assert status != 0 and b"stencil_gcr_decide_batch" in err and text in err, (change, err)
    # (the modes that count need `counts`; the scalar modes do not look at partials or counts)
    status, err = decide_call(mode=c_int(3), counts=None)
    assert status != 0 and b"null pointer" in err


# ------------------------------------------------------------------------------------------------------- the driver
class UnprobedProblem:
    """A member whose operator must not be looked at: every refusal below comes first."""

    def __init__(self, domain):
        self.domain = domain

    def __getattr__(self, name):
        raise AssertionError("the member was probed ({})".format(name))


class ProbedProblem:
    """A member that is no recognised Poisson operator and is never linearised."""

    _fused = None

    def __init__(self, domain):
        self.domain = domain

    def recognise(self, state):
        return None


def _members(monkeypatch, n, kind=UnprobedProblem, nb=3):
    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    domains = [odil.Domain(cshape=[n], multigrid=False, dtype=np.float64) for _ in range(nb)]
    problems = [kind(domain) for domain in domains]
    return odil, problems, [domain.init_state(odil.State(fields={"u": None})) for domain in domains]


ARGS = dict(epoch_start=0, epochs=1, linsolver="multigrid", linsolver_tol=1e-10)


def test_the_driver_names_the_three_values(monkeypatch):
    odil, problems, states = _members(monkeypatch, 8)
    with pytest.raises(ValueError, match="krylov 'sometimes' is neither 'never' nor 'auto' nor 'any'"):
        odil.util.optimize_newton_ensemble(argparse.Namespace(**ARGS), problems, states, krylov="sometimes")


def test_any_passes_the_structural_checks_without_probing(monkeypatch):
    """The shapes are judged before any operator is probed: a form that refuses the shape says so with a ValueError, and
    where the shapes pass -- 'any' is no reason to refuse the batched launches -- the first thing that fails is the probe."""
    odil, problems, states = _members(monkeypatch, 65536)
    args = argparse.Namespace(**ARGS)
    with pytest.raises(ValueError, match="member 0.*65536 cells"):  # (form 'workgroup': its own refusal)
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="any")
    for form in ("auto", "launches"):
        with pytest.raises(AssertionError, match="the member was probed"):
            odil.util.optimize_newton_ensemble(args, problems, states, krylov="any", form=form)
    # 'auto' keeps its refusals
    with pytest.raises(ValueError, match=r"no hand-over to GCR \(krylov 'auto'\)"):
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="auto", form="auto")
    with pytest.raises(ValueError, match="krylov 'auto' with form 'launches'"):
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="auto", form="launches")
    odil, problems, states = _members(monkeypatch, 3)
    with pytest.raises(ValueError, match="member 0.*4 cells per axis"):
        odil.util.optimize_newton_ensemble(args, problems, states, krylov="any", form="launches")


@pytest.mark.parametrize("form", ["launches", "auto"])
def test_the_work_memory_is_checked_for_any_with_the_batched_launches(monkeypatch, form):
    """B (2 m + 2) finest-level vectors, checked by `_krylov_memory_refusal` before any state changes (the members are on
    the host here: the check is made for a device whose free memory is one byte short)."""
    from odil_amd import ensemble

    odil, problems, states = _members(monkeypatch, 65536, kind=ProbedProblem)
    before = [state.fields["u"].array.clone() for state in states]
    need = 3 * 14 * 65536 * 8
    consulted = []
    real = ensemble._krylov_memory_refusal

    def refusal(nbatch, cshape, dtype, device, m):
        consulted.append((nbatch, tuple(cshape), dtype, m))
        return real(nbatch, cshape, dtype, torch.device("cuda:0"), m)

    monkeypatch.setattr(ensemble, "_krylov_memory_refusal", refusal)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (need - 1, 1 << 40))
    with pytest.raises(ValueError, match="{} bytes of work memory, {} bytes of device".format(need, need - 1)):
        odil.util.optimize_newton_ensemble(argparse.Namespace(**ARGS), problems, states, krylov="any", form=form)
    assert consulted == [(3, (65536,), torch.float64, 6)]
    assert all(torch.equal(state.fields["u"].array, u) for state, u in zip(states, before))


def test_the_solver_class_refuses_nine_directions_and_the_newton_step():
    from odil_amd import gmg

    coeffs = torch.zeros((2, 3, 8), dtype=torch.float64)
    with pytest.raises(ValueError, match="EnsembleLaunchKrylovGMG: krylov_m = 9"):
        gmg.EnsembleLaunchKrylovGMG.from_coeffs(coeffs, krylov_m=9)
    with pytest.raises(ValueError, match="EnsembleLaunchKrylovGMG: krylov_m = 0"):
        gmg.EnsembleLaunchKrylovGMG(coeffs, krylov_m=0)
    assert issubclass(gmg.EnsembleLaunchKrylovGMG, gmg.EnsembleLaunchGMG)
    ens = gmg.EnsembleLaunchKrylovGMG.__new__(gmg.EnsembleLaunchKrylovGMG)
    with pytest.raises(ValueError, match="newton_step is not served"):
        ens.newton_step(None, None)
    ens.wpre, ens.wpost, ens.inv = [0.8, 0.8], [0.8, 0.8], torch.zeros((2, 4, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match="_set_cycle: 1 weights for wpre"):  # (the hook of the breakdown test)
        ens._set_cycle(wpre=[0.0])
    with pytest.raises(ValueError, match="_set_cycle: 3 weights for wpost"):
        ens._set_cycle(wpost=[0.0] * 3)
    with pytest.raises(ValueError, match="_set_cycle: inverses"):
        ens._set_cycle(inv=torch.zeros((2, 2, 2), dtype=torch.float64))
    # the base class keeps its refusal
    with pytest.raises(ValueError, match="EnsembleLaunchGMG: krylov 'auto'"):
        gmg.EnsembleLaunchGMG.from_coeffs(coeffs, krylov="auto")


def test_the_example_takes_the_new_value():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
    import ensemble

    assert ensemble.parse_args(["--krylov", "any"]).krylov == "any"
    with pytest.raises(SystemExit):
        ensemble.parse_args(["--krylov", "sometimes"])


# -------------------------------------------------------------------------------------------------------- the model
LEVELS = {"A": [(64,), (32,), (16,), (8,), (4,), (2,)], "B": [(8, 8, 8), (4, 4, 4), (4, 2, 2)]}


@pytest.mark.parametrize("case", model.CASES, ids=["A-1d-64", "B-8^3"])
def test_the_levels_of_the_cases_and_their_splits(case):
    """tail_max_cells = 16: two launch levels (in case B the transition between them is followed by one that merges some
    axes only, and the tail is its one level); tail_max_cells = 64: one launch level."""
    from odil_amd.gmg import EnsembleLaunchGMG as G

    coeffs, _ = model.case_arrays(case)
    for c in coeffs:
        assert model.level_shapes(list(c)) == LEVELS[case[0]]
    levels = LEVELS[case[0]]
    assert G.split(levels, 16) == 2 and G.split(levels, 64) == 1
    if case[0] == "B":
        assert levels[2] == (4, 2, 2)  # (axis 0 is kept: the residual + mean_children path on launch level 1)
