"""The ensemble of small Poisson problems (odil_poisson_small_epochs_batch, util.optimize_ensemble) as far as it can be
checked without a device: the library exports the batched entry points, their launcher refuses malformed arguments with
an error text before anything is launched (the pointers are dummies; tests/test_cabi.py is the model), and
`optimize_ensemble` names the first member that cannot join an ensemble.  (A member whose operator is not the Poisson
stencil is found by probing the operator on the device: tests/test_ensemble_gpu.py.)"""

import argparse
import os
import sys
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_batch_entry_points():
    from odil_amd import _lib

    lib = _lib.load()
    for name in ("odil_poisson_small_epochs_batch_f64", "odil_poisson_small_epochs_batch_f32",
                 "odil_poisson_small_epochs_partials"):
        assert hasattr(lib, name) and name in _lib.EXPORTED, name
    # the reduction workspace of a member: five doubles per workgroup of the residual kernel's schedule
    assert lib.odil_poisson_small_epochs_partials(_lib.i64([256]), 1, 8) == 5
    assert lib.odil_poisson_small_epochs_partials(_lib.i64([256]), 1, 4) == 5
    assert lib.odil_poisson_small_epochs_partials(_lib.i64([40, 94]), 2, 8) >= 5
    assert lib.odil_poisson_small_epochs_partials(_lib.i64([256]), 3, 8) == 0
    assert lib.odil_poisson_small_epochs_partials(None, 1, 8) == 0


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_batch_launcher_refuses_before_launching(suffix):
    """Null pointers, B < 1, strides smaller than a member, levels that do not halve and a partials workspace that is too
    small: ODIL_E_INVAL with a text that names the entry point and the reason.  Every pointer is a dummy, so a launch
    that did happen could not succeed; none is attempted (no device is needed for this test to pass)."""
    from odil_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, "odil_poisson_small_epochs_batch_" + suffix)
    real = float  # (the bindings convert to the entry point's real type)
    shapes = [(16, 8), (8, 4), (4, 2)]  # 128 + 32 + 8 = 168 unknowns, 128 cells
    total, cells, nep = 168, 128, 7
    npart = lib.odil_poisson_small_epochs_partials(_lib.i64(shapes[0]), 2, 8 if suffix == "f64" else 4)
    assert npart >= 5
    steps = np.array([0.25, 0.5], dtype=np.float64 if suffix == "f64" else np.float32)

    def launch(nbatch=3, state=total, field=cells, shp=shapes, ndim=2, alpha=nep, nepochs=nep, out=nep, part=npart, null=None):
        # x m v g u fu rhs | h2 | alphas | losses norms | partials: dummies, but for h2, which is a HOST array the launcher reads
        ptrs = [c_void_p(4096 * (k + 1)) for k in range(12)]
        ptrs[7] = steps.ctypes.data_as(c_void_p)
        flat = _lib.i64([n for s in shp for n in s])
        if null is not None:
            if null == 12:
                flat = None
            else:
                ptrs[null] = None
        x, m, v, g, u, fu, rhs, h2, alphas, losses, norms, partials = ptrs[:12]
        return fn(x, m, v, g, u, fu, rhs, c_int(nbatch), c_int64(state), c_int64(field), flat, c_int(len(shp)), c_int(ndim),
                  h2, alphas, c_int64(alpha), c_int(nepochs), real(0.1), real(0.001), real(1e-7), losses, norms,
                  c_int64(out), partials, c_int64(part), None)

    def refused(text, **kw):
        assert launch(**kw) == -1, kw
        err = lib.odil_last_error()
        assert b"poisson_small_epochs_batch" in err and text in err, (kw, err)

    for k in range(13):
        refused(b"null pointer", null=k)
    for nbatch in (0, -1):
        refused(b"members", nbatch=nbatch)
    refused(b"smaller than a member", state=total - 1)
    refused(b"smaller than a member", field=cells - 1)
    refused(b"smaller than a member", state=0)
    refused(b"smaller than", alpha=nep - 1)  # (0 = one table for all members is allowed; anything else holds a row)
    refused(b"smaller than", out=nep - 1)
    refused(b"smaller than", out=0)
    refused(b"does not halve", shp=[(16, 8), (8, 4), (4, 3)])
    refused(b"does not halve", shp=[(16, 8), (7, 4)])
    refused(b"does not halve", shp=[(94,), (47,), (23,)], ndim=1, state=164, field=94)
    refused(b"too small", part=npart - 1)
    refused(b"too small", part=0)
    refused(b"epochs", nepochs=0)
    refused(b"ndim 3", ndim=3)


# ------------------------------------------------------------------------------------------- optimize_ensemble
@pytest.fixture()
def api(monkeypatch):
    """(odil, the Poisson example) with the process-wide `mod` on CPU tensors: problems and states can be built, nothing
    can be computed (ModRocm(device='cpu') exists for this kind of plumbing check)."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    return odil, poisson


def stretched(odil, poisson):
    """The 1-D N = 64 problem on a box twice as long: same shapes, another spacing."""
    domain = odil.Domain(cshape=[64], multigrid=True, dtype=np.float64, upper=2.0)
    state = domain.init_state(odil.State(fields={"u": None}))
    extra = argparse.Namespace(rhs=domain.points()[0] * 0, args=argparse.Namespace(mgloss=0))
    return odil.Problem(poisson.operator, domain, extra), state


def members(odil, poisson, specs):
    out = [stretched(odil, poisson) if spec == "stretched" else poisson.make_problem(poisson.parse_args(spec.split()))
           for spec in specs]
    args = poisson.parse_args(specs[0].split())
    args.epoch_start, args.epochs = 0, 5
    return args, [p for p, _ in out], [s for _, s in out]


def test_optimize_ensemble_exists_and_wants_adam(api):
    odil, poisson = api
    args, problems, states = members(odil, poisson, ["--ndim 1 --N 64"] * 2)
    for optname in ("lbfgsb", "gd", "newton"):
        args.optimizer = optname
        with pytest.raises(ValueError, match="Adam.*'{}'".format(optname)):
            odil.util.optimize_ensemble(args, problems, states)
    args.optimizer = "adam"
    with pytest.raises(ValueError, match="3 step sizes for 2 members"):
        odil.util.optimize_ensemble(args, problems, states, lrs=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="2 problems with 1 states"):
        odil.util.optimize_ensemble(args, problems, states[:1])


@pytest.mark.parametrize("specs,member,reason", [
    (["--ndim 1 --N 64", "--ndim 1 --N 64", "--ndim 1 --N 128"], 2, "level shapes .* differ from member 0"),
    (["--ndim 2 --N 16", "--ndim 1 --N 16"], 1, "level shapes .* differ from member 0"),
    (["--ndim 1 --N 64", "--ndim 1 --N 64 --multigrid 0"], 1, "level shapes .* differ from member 0"),
    (["--ndim 2 --N 16", "--ndim 3 --N 16", "--ndim 1 --N 8192"], 1, "3-D grid"),
    (["--ndim 3 --N 8"], 0, "3-D grid"),
    (["--ndim 1 --N 256", "--ndim 1 --N 8192 --multigrid 0"], 1, "8192 cells are above the limit"),
    (["--ndim 1 --N 8192"], 0, "13 levels"),
    (["--ndim 2 --N 128"], 0, "16384 cells are above the limit"),
    (["--ndim 1 --N 64 --double 0", "--ndim 1 --N 64"], 1, "dtype"),
    (["--ndim 1 --N 64", "--ndim 1 --N 64", "stretched"], 2, "grid spacing"),
], ids=["mixed-size", "mixed-ndim", "mixed-levels", "3d-member", "3d-alone", "above-limit-1d", "too-many-levels",
        "above-limit-2d", "mixed-dtype", "mixed-spacing"])
def test_optimize_ensemble_names_the_first_offending_member(api, specs, member, reason):
    """Members that cannot run side by side raise ValueError with their index and the reason -- from the shapes alone,
    before any operator is probed (so before any device is needed)."""
    odil, poisson = api
    args, problems, states = members(odil, poisson, specs)
    with pytest.raises(ValueError, match="member {}: .*{}".format(member, reason)):
        odil.util.optimize_ensemble(args, problems, states)


def test_small_refusal_is_the_predicate_of_small_plan():
    """`fused.small_refusal` (what optimize_ensemble asks) and `PoissonEvaluator.small_plan` admit the same levels."""
    from odil_amd import fused

    f64, f32 = torch.float64, torch.float32
    assert fused.small_refusal([(256,), (128,)], f64) is None
    assert fused.small_refusal([(4096,)], f64) is None and "limit" in fused.small_refusal([(8192,)], f64)
    assert fused.small_refusal([(32, 32), (16, 16)], f64) is None
    assert "limit" in fused.small_refusal([(40, 94), (20, 47)], f64) and fused.small_refusal([(40, 94), (20, 47)], f32) is None
    assert fused.small_refusal([(40, 94), (20, 47)], f64, force=True) is None
    assert "halve" in fused.small_refusal([(94,), (47,), (23,)], f64)
    assert "switched off" in fused.small_refusal([(256,)], f64, max_cells=0)
    assert "3-D" in fused.small_refusal([(8, 8, 8)], f64)
