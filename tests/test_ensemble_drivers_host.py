"""The ensemble drivers of odil_amd/ensemble.py as far as they can be checked without a device: `util` exports the drivers of
that module, ONE member check serves both drivers, ONE loop serves both Newton routes (driven with a solver that only
records its calls), and every `gmg.EnsembleGMG` ends its construction with the attributes its docstring lists."""

import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def api(monkeypatch):
    """(odil, the Poisson example) with the process-wide `mod` on CPU tensors: problems and states can be built, nothing
    can be computed."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    return odil, poisson


def test_util_exports_the_drivers_of_the_ensemble_module(api):
    odil, _ = api
    assert odil.util.optimize_ensemble is odil.ensemble.optimize_ensemble
    assert odil.util.optimize_newton_ensemble is odil.ensemble.optimize_newton_ensemble
    assert odil.optimize is odil.util.optimize and not hasattr(odil.util, "_newton_ensemble_stencil")


# ------------------------------------------------------------------------------------------------ one member check
BASE = "--multigrid 0 --ndim 1 --N 64 "


def stretched(odil, poisson):
    """The 1-D N = 64 problem with a plain unknown on a box twice as long: same shape, another spacing."""
    domain = odil.Domain(cshape=[64], multigrid=False, dtype=np.float64, upper=2.0)
    state = domain.init_state(odil.State(fields={"u": None}))
    extra = argparse.Namespace(rhs=domain.points()[0] * 0, args=argparse.Namespace(mgloss=0))
    return odil.Problem(poisson.operator, domain, extra), state


@pytest.mark.parametrize("second,reason", [("stretched", "grid spacing"), ("--double 0", "dtype")],
                         ids=["mixed-spacing", "mixed-dtype"])
def test_both_drivers_name_the_same_member_with_their_own_prefix(api, second, reason):
    odil, poisson = api
    make = lambda spec: poisson.make_problem(poisson.parse_args((BASE + spec).split()))
    built = [make(""), stretched(odil, poisson) if second == "stretched" else make(second)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    args = poisson.parse_args((BASE + "--linsolver multigrid").split())
    args.epoch_start, args.epochs, args.optimizer = 0, 2, "adam"
    for driver in ("optimize_ensemble", "optimize_newton_ensemble"):
        with pytest.raises(ValueError, match="^{}: member 1: {} .* differ from member 0's".format(driver, reason)):
            getattr(odil.util, driver)(args, problems, states)


# --------------------------------------------------------------------------------------------------- one Newton loop
NB, N, EPOCHS = 3, 64, 4


def recording_solver(gmg):
    """A gmg.EnsembleGMG (its limits and `plan` are host arithmetic) that records what the driver asks of it instead of
    launching anything; `calls` belongs to the class: the driver constructs the solver itself."""

    class RecordingSolver(gmg.EnsembleGMG):
        calls = []

        def __init__(self, *args):
            self.outcome = np.zeros((NB, 2), dtype=np.int32)
            self.coarse = torch.zeros((NB, 3, N), dtype=torch.float64)
            self.calls.append("made")

        from_coeffs = classmethod(lambda cls, coeffs: cls(coeffs))
        fine = property(lambda self: self.coarse)

        def _step(self, name):
            self.calls.append(name)
            self.outcome[:, 0] = self.calls.count(name)  # (the "cycles" of this step: its number)

        def newton_step(self, u, rhs, tol, maxcycles):
            self._step("newton_step")

        def solve(self, b, x, tol, maxcycles, start):
            self._step("solve")

        def rebuild(self):
            self.calls.append("rebuild")

        def status(self, member):
            return dict(residual=0.25 * (member + 1), niter=int(self.outcome[member, 0]), converged=True)

    return RecordingSolver


class ConstantProblem:
    """A member that computes nothing: constant loss, a zero linearisation; `poisson`: whether it counts as recognised."""

    def __init__(self, domain, poisson):
        self.domain = domain
        self._fused = argparse.Namespace(nlvl=1, cshape=(N,), h2=[1.0 / N ** 2], dtype=torch.float64, device=None,
                                         rhs=torch.zeros(N, dtype=torch.float64)) if poisson else None

    def recognise(self, state):
        pass

    def eval_loss_grad_device(self, state):
        one = torch.ones(())
        return one, None, [one], ["f"], [one]

    def linearize_device(self, state):
        return torch.zeros(N, dtype=torch.float64), None


def stub_members(odil, monkeypatch, route):
    """(problems, states, the calls the solver will record) of NB members that take `route`."""
    solver = recording_solver(odil.gmg)
    monkeypatch.setattr(odil.gmg, "EnsembleGMG", solver)
    monkeypatch.setattr(odil.gmg, "recognise_stencil", lambda matrix: torch.zeros((3, N), dtype=torch.float64))
    monkeypatch.setattr(odil.ops, "axpy", lambda x, y, a: x.add_(y, alpha=a))
    domains = [odil.Domain(cshape=[N], multigrid=False, dtype=np.float64) for _ in range(NB)]
    problems = [ConstantProblem(domain, route == "poisson" or b == 0) for b, domain in enumerate(domains)]
    return problems, [domain.init_state(odil.State(fields={"u": None})) for domain in domains], solver.calls


@pytest.mark.parametrize("cadence", [1, 3])
def test_the_newton_routes_share_the_loop(api, monkeypatch, cadence):
    """Both routes of `optimize_newton_ensemble`, with the solver and the device work replaced: the callback comes at the
    epochs its `next_active` names, with the solver's status after a step, and the tables have a column per epoch."""
    odil, _ = api
    args = argparse.Namespace(epoch_start=0, epochs=EPOCHS, linsolver="multigrid", linsolver_tol=1e-10)
    seen = dict()
    for route in ("poisson", "stencil"):
        problems, states, calls = stub_members(odil, monkeypatch, route)  # (stencil: one member is not the Poisson operator)
        reports = []

        def callback(member, state, epoch, pinfo):
            assert state is states[member]
            reports.append((member, epoch, pinfo.get("linsolver")))

        if cadence > 1:
            callback.next_active = lambda epoch: (epoch // cadence + 1) * cadence
        arrays, info = odil.util.optimize_newton_ensemble(args, problems, states, callback)
        assert info.route == route and info.epochs == EPOCHS and info.evals == EPOCHS and len(arrays) == NB
        assert info.cycles.shape == (NB, EPOCHS) and info.residuals.shape == (NB, EPOCHS)
        assert (info.cycles == np.arange(1, EPOCHS + 1)).all() and (info.residuals[:, 0] == [0.25, 0.5, 0.75]).all()
        steps = ["newton_step"] * EPOCHS if route == "poisson" else ["solve"] + ["rebuild", "solve"] * (EPOCHS - 1)
        assert calls == ["made"] + steps
        for member, epoch, status in reports:  # (no status at the start, the member's own after a step)
            assert (status is None) == (epoch == 0) and (epoch == 0 or status["residual"] == 0.25 * (member + 1))
        base = states[0].fields["u"].array.untyped_storage().data_ptr()
        assert all(state.fields["u"].array.untyped_storage().data_ptr() == base for state in states)  # (views of one u)
        seen[route] = [(member, epoch) for member, epoch, _ in reports]
    epochs = [0, 1, 2, 3, 4] if cadence == 1 else [0, 3]
    assert seen["poisson"] == seen["stencil"] == [(member, epoch) for epoch in epochs for member in range(NB)]


def test_the_stencil_route_builds_no_solver_without_an_epoch(api, monkeypatch):
    odil, _ = api
    problems, states, calls = stub_members(odil, monkeypatch, "stencil")
    args = argparse.Namespace(epoch_start=2, epochs=2, linsolver="direct")
    arrays, info = odil.util.optimize_newton_ensemble(args, problems, states)
    assert info.solver is None and info.route == "stencil" and info.cycles.shape == (NB, 0) and calls == []


# ------------------------------------------------------------------------------------------- one kind of EnsembleGMG
def test_every_ensemble_gmg_ends_with_the_documented_core(monkeypatch):
    """The attributes the class docstring promises are the tuple `core`, and `_finish` -- the end of every construction --
    asserts them: every object made on a device checks itself."""
    from odil_amd import gmg, ops

    cls = gmg.EnsembleGMG
    listed = re.search(r"\n\s+(nbatch, [\w, ]+)\n", cls.__doc__).group(1)
    assert tuple(listed.split(", ")) == cls.core
    monkeypatch.setattr(ops, "stencil_solve_batch_plan", lambda *args: None)
    shapes, halves = [(8,), (4,)], [[True]]
    coeffs, inv = torch.zeros(3 * 12, dtype=torch.float64), torch.zeros((4, 4), dtype=torch.float64)
    bare = cls.__new__(cls)
    bare.nbatch, bare.dtype, bare.device, bare.wpre, bare.wpost = 2, torch.float64, None, [1.0], [1.0]
    with pytest.raises(AssertionError, match="ndim.*nu1.*nu2.*method"):
        bare._finish(shapes, halves, coeffs, inv)
    bare.ndim, bare.nu1, bare.nu2, bare.method = 1, 1, 1, "stub"
    bare._finish(shapes, halves, coeffs, inv)
    assert bare.locs == ["c"] and bare.cells == 8 and tuple(bare.work.shape) == (2, 3 * 12) and bare.outcome is None
    with pytest.raises(ValueError, match="not walked by one workgroup"):
        bare._finish([(1024,)], [], coeffs, inv)
    assert bare.shapes == shapes  # (a refused set of levels changes nothing)
    bare._strength = None
    for call in (lambda: bare.fine, lambda: bare.level(0), bare.rebuild):
        with pytest.raises(ValueError, match="only an object made by from_coeffs"):
            call()
