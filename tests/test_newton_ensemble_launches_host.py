"""Newton ensembles of members beyond one workgroup, what needs no device: `fused.newton_launches_refusal`, the split of a
hierarchy into launch levels and a one-workgroup tail (`gmg.EnsembleLaunchGMG.split` / `plan`), the refusals of the
batched cycle entry points (odil_stencil_var_smooth_batch, odil_stencil_var_residual_restrict_batch,
odil_stencil_cycle_decide_batch: ODIL_E_INVAL before any launch, the pointers are dummies) and the `form` argument of
`optimize_newton_ensemble`."""

import os
import sys
from ctypes import c_double, c_int, c_int64, c_void_p

import pytest
import torch
from conftest import ROOT

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------------ the refusals
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("shape", [(256, 256), (64, 64, 64), (65536,), (256, 160), (40, 32, 32)], ids=str)
def test_newton_launches_refusal_admits(shape, dtype):
    from odil_amd import fused

    assert fused.newton_launches_refusal(shape, dtype) is None


def test_newton_launches_refusal_gives_each_reason():
    from odil_amd import fused

    assert "4-D" in fused.newton_launches_refusal((8,) * 4, F64)
    assert "0-D" in fused.newton_launches_refusal((), F64)
    assert "4 cells per axis" in fused.newton_launches_refusal((256, 3), F64)
    assert "4 cells per axis" in fused.newton_launches_refusal((2, 64, 64), F32)
    assert "dtype" in fused.newton_launches_refusal((256, 256), torch.float16)
    assert "dtype" in fused.newton_launches_refusal((256, 256), torch.int32)
    assert "limit per member" in fused.newton_launches_refusal((4096, 8192), F64)
    # 250^2 -> 125^2: a tail of one level with 15625 unknowns; 502^2 -> 251^2 = 63001 cells: no level for a tail at all
    assert "coarsest level of at most 512 unknowns" in fused.newton_launches_refusal((250, 250), F64)
    assert "no level of at most 32768 cells" in fused.newton_launches_refusal((502, 502), F64)


def test_the_one_workgroup_refusals_keep_their_texts():
    from odil_amd import fused

    for shape, cells in (((256, 256), 65536), ((64,) * 3, 262144)):
        want = "{} cells are above the limit of the one-workgroup Newton solves (32768)".format(cells)
        assert fused.newton_stencil_refusal(shape, F64) == want
        assert fused.newton_refusal(shape, [1.0 / shape[0] ** 2] * len(shape), F64) == want


# ----------------------------------------------------------------------------------------------------- the level split
def test_level_split_is_host_arithmetic():
    from odil_amd.gmg import EnsembleLaunchGMG as G

    launch, tail = G.plan((256, 160))
    assert launch == [(256, 160)] and tail == [(128, 80), (64, 40), (32, 20), (16, 10), (8, 5)]
    launch, tail = G.plan((40, 32, 32))
    assert launch == [(40, 32, 32)] and tail == [(20, 16, 16), (10, 8, 8), (5, 4, 4)]
    launch, tail = G.plan((128,) * 3)
    assert launch == [(128,) * 3, (64,) * 3] and tail[0] == (32,) * 3 and tail[-1] == (2,) * 3
    launch, tail = G.plan((16, 16), tail_max_cells=64)
    assert launch == [(16, 16)] and tail == [(8, 8), (4, 4), (2, 2)]
    launch, tail = G.plan((32, 32), tail_max_cells=64)
    assert launch == [(32, 32), (16, 16)] and tail == [(8, 8), (4, 4), (2, 2)]
    # the finest level is a launch level however small it is
    launch, tail = G.plan((8, 8))
    assert launch == [(8, 8)] and tail == [(4, 4), (2, 2)]
    # a long 1-D tail stops after max_levels levels
    launch, tail = G.plan((65536,))
    assert launch == [(65536,)] and len(tail) == G.max_levels == 8 and tail[-1] == (256,)
    assert G.split([(16, 16), (8, 16), (4, 16), (2, 16)], 64) == 2  # (semi-coarsened levels: by their cells alone)


def test_levels_that_do_not_split_are_refused_by_name():
    from odil_amd.gmg import EnsembleLaunchGMG as G

    nine = [(2 ** k,) for k in range(17, 7, -1)]  # 131072, then a tail of 9 levels 65536 ... 256
    with pytest.raises(ValueError, match=r"the tail \[\(65536,\).*\(256,\)\].*at most 8 levels"):
        G.split(nine, 65536)
    with pytest.raises(ValueError, match=r"the tail \[\(125, 125\)\] of the levels \[\(250, 250\), \(125, 125\)\].*at most 512"):
        G.split([(250, 250), (125, 125)])
    with pytest.raises(ValueError, match=r"levels \[\(502, 502\), \(251, 251\)\] have no level of at most 32768 cells"):
        G.split([(502, 502), (251, 251)])
    with pytest.raises(ValueError, match="coarsest level of at most 512"):
        G.plan((100, 100))  # 100 -> 50 -> 25: 625 unknowns
    with pytest.raises(ValueError, match="coarsest level of at most 512"):
        G.plan((1 << 18,), tail_max_cells=1 << 17)  # 8 levels from 131072 end at 1024


# ------------------------------------------------------------------------------------ the entry points' own refusals
class Launchers:
    """The three entry points with dummy pointers; every keyword replaces one well-formed argument."""

    def __init__(self, suffix):
        from odil_amd import _lib

        self.lib, self.i64 = _lib.load(), _lib.i64
        self.real = c_double if suffix == "f64" else __import__("ctypes").c_float
        self.fn_smooth = getattr(self.lib, "odil_stencil_var_smooth_batch_" + suffix)
        self.fn_restrict = getattr(self.lib, "odil_stencil_var_residual_restrict_batch_" + suffix)

    P = dict(coeffs=4096, x=8192, b=12288, out=16384, active=20480, partials=24576)

    def smooth(self, shape=(8, 12), ndim=None, nbatch=3, mode=0, cs=None, xs=None, bs=None, os_=None, null=(), same=False,
               partials=False):
        cells = 1
        for n in shape:
            cells *= n
        p = {k: (None if k in null else c_void_p(v)) for k, v in self.P.items()}
        if same:
            p["out"] = p["x"]
        return self.fn_smooth(p["coeffs"], c_int64((2 * len(shape) + 1) * cells + 2 if cs is None else cs), p["x"],
                              c_int64(cells if xs is None else xs), p["b"], c_int64(cells if bs is None else bs), p["out"],
                              c_int64(cells if os_ is None else os_), None if "shape" in null else self.i64(shape),
                              c_int(len(shape) if ndim is None else ndim), c_int(nbatch), self.real(0.8), c_int(mode),
                              p["active"], p["partials"] if partials else None, None)

    def restrict(self, shape=(8, 12), ndim=None, nbatch=3, cs=None, xs=None, bs=None, os_=None, null=()):
        cells = 1
        for n in shape:
            cells *= n
        p = {k: (None if k in null else c_void_p(v)) for k, v in self.P.items()}
        return self.fn_restrict(p["coeffs"], c_int64((2 * len(shape) + 1) * cells + 2 if cs is None else cs), p["x"],
                                c_int64(cells if xs is None else xs), p["b"], c_int64(cells if bs is None else bs), p["out"],
                                c_int64(cells // 2 ** len(shape) if os_ is None else os_),
                                None if "shape" in null else self.i64(shape), c_int(len(shape) if ndim is None else ndim),
                                c_int(nbatch), self.real(0.25), p["active"], None)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_batched_cycle_launchers_refuse_before_launching(suffix):
    run = Launchers(suffix)
    names = dict(smooth=b"stencil_var_smooth_batch", restrict=b"stencil_var_residual_restrict_batch")

    def refused(which, text, **kw):
        assert getattr(run, which)(**kw) == -1, (which, kw)
        err = run.lib.odil_last_error()
        assert names[which] in err and text in err, (which, kw, err)

    cells = 96
    for which in ("smooth", "restrict"):
        for null in ("coeffs", "b", "out", "shape"):
            refused(which, b"null pointer", null=(null,))
        refused(which, b"0 members", nbatch=0)
        refused(which, b"65536 members", nbatch=65536)
        refused(which, b"ndim 4", shape=(4, 4, 4, 4), ndim=4)
        refused(which, b"ndim 0", ndim=0)
        refused(which, b"empty extent", shape=(8, 0))
        refused(which, b"coeff_stride", cs=5 * cells - 1)
        refused(which, b"x_stride", xs=cells - 1)
        refused(which, b"b_stride", bs=cells - 1)
    refused("smooth", b"out_stride", os_=cells - 1)
    refused("restrict", b"coarse_stride", os_=cells // 4 - 1)
    # the sweep: not in place, x only optional for the sweep itself, partial sums with the sweep only, two modes
    refused("smooth", b"in-place", same=True)
    refused("smooth", b"null pointer", null=("x",), mode=1)
    refused("smooth", b"partial sums go with mode 0", mode=1, partials=True)
    refused("smooth", b"mode 2", mode=2)
    # the restricted residual: x is required, every extent even, even strides between members
    refused("restrict", b"null pointer", null=("x",))
    refused("restrict", b"not even", shape=(8, 13))
    refused("restrict", b"not even", shape=(7,))
    refused("restrict", b"not even", shape=(4, 6, 5))
    refused("restrict", b"odd stride", xs=cells + 1)
    refused("restrict", b"odd stride", cs=5 * cells + 1)


def test_smooth_batch_parts():
    from odil_amd import _lib, ops

    assert ops.stencil_var_smooth_batch_parts((64,)) == 1
    assert ops.stencil_var_smooth_batch_parts((12, 20)) == 1
    assert ops.stencil_var_smooth_batch_parts((16, 16, 16)) == 16
    assert ops.stencil_var_smooth_batch_parts((256, 160)) == 160
    assert ops.stencil_var_smooth_batch_parts((257,)) == 2
    lib = _lib.load()
    for shape in [(0,), (8, 0), (-4, 4), (4, 4, 4, 4), (), (1 << 13, 1 << 12)]:
        assert lib.odil_stencil_var_smooth_batch_parts(_lib.i64(shape or [1]), c_int(len(shape))) == 0, shape
    assert lib.odil_stencil_var_smooth_batch_parts(None, c_int(2)) == 0


def test_cycle_decide_refuses_before_launching():
    from odil_amd import _lib

    lib = _lib.load()
    ptrs = dict(partials=4096, partials0=8192, history=12288, outcome=16384, active=20480, nactive=24576)

    def decide(null=(), pstride=4, p0stride=4, nparts=4, nbatch=3, cells=1024, k=1, maxcycles=5, tol=1e-8, hstride=7,
               with0=True):
        p = {name: (None if name in null else c_void_p(v)) for name, v in ptrs.items()}
        return lib.odil_stencil_cycle_decide_batch(
            p["partials"], c_int64(pstride), p["partials0"] if with0 else None, c_int64(p0stride), c_int(nparts), c_int(nbatch),
            c_int64(cells), c_int(k), c_int(maxcycles), c_double(tol), p["history"], c_int64(hstride), p["outcome"], p["active"],
            p["nactive"], None)

    def refused(text, **kw):
        assert decide(**kw) == -1, kw
        err = lib.odil_last_error()
        assert b"stencil_cycle_decide_batch" in err and text in err, (kw, err)

    for null in ("partials", "history", "outcome", "active", "nactive"):
        refused(b"null pointer", null=(null,))
    refused(b"0 members", nbatch=0)
    refused(b"65536 members", nbatch=65536)
    refused(b"partial sums", nparts=0)
    refused(b"partial sums", pstride=3)
    refused(b"partial sums", p0stride=3)
    refused(b"partial sums", cells=0)
    refused(b"cycle 6 of at most 5", k=6)
    refused(b"cycle -1", k=-1)
    refused(b"history_stride", hstride=6)
    refused(b"tolerance", tol=-1.0)
    refused(b"tolerance", tol=float("nan"))


# ------------------------------------------------------------------------------------------ optimize_newton_ensemble
@pytest.fixture()
def api(monkeypatch):
    """(odil, the diffusion ensemble example) with the process-wide `mod` on CPU tensors: problems and states can be
    built, nothing can be computed."""
    sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
    import ensemble

    import odil_amd as odil

    monkeypatch.setattr(odil.runtime, "_mod", odil.ModRocm(device="cpu"))
    monkeypatch.setattr(odil.util, "g_log_file", open(os.devnull, "w"))
    return odil, ensemble


def members(ensemble, specs):
    built = []
    for b, spec in enumerate(specs):
        args = ensemble.parse_args(spec.split() + ["--members", str(len(specs))])
        built.append(ensemble.make_member(args, b))
    args = ensemble.parse_args(specs[0].split())
    args.epoch_start, args.epochs = 0, 2
    return args, [p for p, _ in built], [s for _, s in built]


def test_an_unknown_form_raises_before_any_member_is_looked_at(api):
    odil, _ = api
    with pytest.raises(ValueError, match="form 'nonsense' is none of 'workgroup', 'launches', 'auto'"):
        odil.util.optimize_newton_ensemble(None, [object()], [], form="nonsense")  # (nothing here could be looked at)


def test_the_default_form_refuses_members_beyond_one_workgroup_as_before(api):
    odil, ensemble = api
    args, problems, states = members(ensemble, ["--ndim 2 --N 256"] * 2)
    before = [s.fields["u"].array.clone() for s in states]
    for kw in (dict(), dict(form="workgroup")):
        with pytest.raises(ValueError, match="optimize_newton_ensemble: member 0: 65536 cells are above the limit of the "
                                             "one-workgroup Newton solves"):
            odil.util.optimize_newton_ensemble(args, problems, states, **kw)
    assert all(torch.equal(s.fields["u"].array, a) for s, a in zip(states, before))


def test_form_launches_names_the_member_it_refuses(api):
    odil, ensemble = api
    args, problems, states = members(ensemble, ["--ndim 2 --N 250"] * 2)
    for form in ("launches", "auto"):
        with pytest.raises(ValueError, match="optimize_newton_ensemble: member 0: .*(coarsest level|625 unknowns)"):
            odil.util.optimize_newton_ensemble(args, problems, states, form=form)
    args, problems, states = members(ensemble, ["--ndim 2 --N 256", "--ndim 2 --N 128"])
    with pytest.raises(ValueError, match="optimize_newton_ensemble: member 1: cells .* differ from member 0"):
        odil.util.optimize_newton_ensemble(args, problems, states, form="launches")


def test_the_example_takes_a_form():
    sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
    import ensemble

    assert ensemble.parse_args([]).form == "workgroup"
    assert ensemble.parse_args(["--form", "launches"]).form == "launches"
    with pytest.raises(SystemExit):
        ensemble.parse_args(["--form", "volumes"])
