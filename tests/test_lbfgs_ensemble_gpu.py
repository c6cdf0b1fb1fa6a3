"""L-BFGS-B ensembles on the device (`odil.util.optimize_ensemble` with args.optimizer == "lbfgsb"): every batched entry
point of the vector algebra against the single one per member (`torch.equal`, same bits), the Poisson adjoint without an
update against `ops.poisson_adjoint`, and whole ensembles against the members' own `optimize_grad(args, "lbfgsb", ...)`
runs -- every level array, every callback report, iteration and evaluation counts and the final task -- in float64 and in
float32 domains, on the traced route (members of tests/traced_ensemble_members.py) and on the Poisson route."""

import argparse
import os
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT
from traced_ensemble_members import make_member

import odil_amd as odil
from odil_amd import ops
from odil_amd.optimizer import EarlyStopError

pytestmark = pytest.mark.gpu

TDTYPES = [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")]
DTYPES = [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")]
NB, ROWS = 5, 6
LIST, COUNTS = [0, 2, 4], (0, 2, 6, 1, 4)
# odd: the scalar path; the pack of 16^2 + 8^2 + 4^2; the first size of the read-once products; a size past it
SIZES = [7, 336, 16384, 16392]


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    saved = odil.util.g_log_file
    odil.util.set_log_file(open(os.devnull, "w"))
    monkeypatch.setenv("ODIL_GRAPH", "0")
    yield
    odil.util.g_log_file = saved


def same_bits(a, b):
    """Equal bit patterns (a NaN equals itself)."""
    kind = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(kind), b.contiguous().view(kind))


def padded(gen, inner, n, dtype):
    """(base, [NB, *inner, n] view): members `pad` elements apart -- a multiple of 16 bytes where n is one (the members
    keep member 0's alignment), any odd gap where the rows are no whole packs anyway."""
    pad = 3 if n % 2 else (2 if dtype == torch.float64 else 4)
    size = int(np.prod(inner, dtype=np.int64)) * n
    base = torch.randn(NB * (size + pad), generator=gen, dtype=torch.float64).to(dtype).cuda()
    strides = [n * int(np.prod(inner[k + 1:], dtype=np.int64)) for k in range(len(inner))] + [1]
    return base, base.as_strided((NB,) + tuple(inner) + (n,), [size + pad] + strides)


def gaps_untouched(base, before, n_member, listed):
    """Everything of `base` outside the listed members' first n_member elements is as it was."""
    stride = base.numel() // NB
    keep = torch.ones(base.numel(), dtype=torch.bool)
    for b in listed:
        keep[b * stride:b * stride + n_member] = False
    keep = keep.cuda()
    return same_bits(base[keep], before[keep])


def member_list(listed):
    return None if listed is None else torch.tensor(listed, dtype=torch.int32).cuda()


def workspace(n, dtype):
    return torch.empty((NB, ops.lbfgs_batch_partials(n, ROWS, dtype)), dtype=torch.float64).cuda()


LISTS = [pytest.param(LIST, id="list-0-2-4"), pytest.param(None, id="all")]


@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("listed", LISTS)
def test_probe_batch_equals_probe_per_member(n, listed, dtype):
    gen = torch.Generator().manual_seed(n)
    (_, g), (_, d) = padded(gen, (), n, dtype), padded(gen, (), n, dtype)
    g[2, n // 2] = float("nan")  # (a NaN must stay visible in all three)
    out = torch.full((NB, 8), -7.0, dtype=dtype).cuda()
    before = out.clone()
    ops.lbfgs_probe_batch(g, d, out[:, 3:], workspace(n, dtype), member_list(listed))
    for b in range(NB):
        if listed is None or b in listed:
            want = ops.lbfgs_probe(g[b], d[b], torch.zeros(3, dtype=dtype).cuda())
            assert same_bits(out[b, 3:6], want), (b, out[b], want)
            assert bool(torch.isnan(out[b, 3:6]).all()) == (b == 2)
        else:
            assert torch.equal(out[b], before[b])
    assert torch.equal(out[:, :3], before[:, :3]) and torch.equal(out[:, 6:], before[:, 6:])


@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("listed", LISTS)
def test_dots3_batch_equals_dots3_per_member(n, listed, dtype):
    gen = torch.Generator().manual_seed(n + 1)
    (_, w) = padded(gen, (ROWS,), n, dtype)
    bs = [padded(gen, (), n, dtype)[1] for _ in range(3)]
    counts = torch.tensor(COUNTS, dtype=torch.int32).cuda()
    for nrhs in (3, 1):
        out = torch.full((NB, 3, ROWS + 1), -7.0, dtype=dtype).cuda()
        ops.lbfgs_dots3_batch(w, counts, ROWS, bs[:nrhs], out, workspace(n, dtype), member_list(listed))
        for b in range(NB):
            count = COUNTS[b] if (listed is None or b in listed) else 0
            if count:
                want = ops.dots3(w[b, :count], [t[b] for t in bs[:nrhs]])
                assert torch.equal(out[b, :, :count], want), (b, nrhs)
                assert nrhs == 3 or not bool(out[b, 1:, :count].any())
            assert bool((out[b, :, count:] == -7.0).all()), b
    # one vector per member: the probe of a direction, <d, d> and <g, d> into the first columns of the table of scalars
    table = torch.full((NB, 8), -7.0, dtype=dtype).cuda()
    ops.lbfgs_dots3_batch(bs[0], None, 1, [bs[0], bs[1]], table[:, :3].unsqueeze(2), workspace(n, dtype), member_list(listed))
    for b in range(NB):
        if listed is None or b in listed:
            want = ops.dots3(bs[0][b][None], [bs[0][b], bs[1][b]])
            assert torch.equal(table[b, :3], want.view(-1)) and bool((table[b, 3:] == -7.0).all())
        else:
            assert bool((table[b] == -7.0).all())


@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("listed", LISTS)
def test_lincomb_batch_equals_lincomb_per_member(n, listed, dtype):
    gen = torch.Generator().manual_seed(n + 2)
    (_, w), (ybase, y) = padded(gen, (ROWS,), n, dtype), padded(gen, (), n, dtype)
    coef = torch.randn((NB, ROWS), generator=gen, dtype=torch.float64).to(dtype).cuda()
    counts = torch.tensor(COUNTS, dtype=torch.int32).cuda()
    for beta in (1.0, 0.5):
        before, old = ybase.clone(), y.clone()
        ops.lbfgs_lincomb_batch(y, beta, w, counts, ROWS, coef, member_list(listed))
        used = list(range(NB)) if listed is None else listed
        for b in used:
            want = old[b].clone()
            if COUNTS[b]:
                ops.lincomb(want, beta, w[b, :COUNTS[b]], coef[b, :COUNTS[b]].contiguous())
            else:
                want = beta * want
            assert torch.equal(y[b], want), (b, beta)
        assert gaps_untouched(ybase, before, n, used)
    assert not torch.equal(y[2], old[2])


@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("listed", LISTS)
def test_axpy_batch_equals_axpy_scale_and_copy_per_member(n, listed, dtype):
    gen = torch.Generator().manual_seed(n + 3)
    (obase, out), (_, y), (_, x) = (padded(gen, (), n, dtype) for _ in range(3))
    alpha = torch.tensor([0.3, -1.0, 1.0, 2.5e-3, -7.0], dtype=dtype).cuda()
    used = list(range(NB)) if listed is None else listed
    for mode in ("axpy", "axpy-in-place", "scale", "copy"):
        before = obase.clone()
        if mode == "axpy":
            ops.lbfgs_axpy_batch(out, y, x, alpha, member_list(listed))
        elif mode == "axpy-in-place":
            old = out.clone()
            ops.lbfgs_axpy_batch(out, out, x, alpha, member_list(listed))
        elif mode == "scale":
            ops.lbfgs_axpy_batch(out, None, x, alpha, member_list(listed))
        else:
            ops.lbfgs_axpy_batch(out, None, x, None, member_list(listed))
        for b in used:
            if mode == "axpy":  # (LbfgsVectors.set_axpy: a copy, then y += a x)
                want = ops.axpy(y[b].clone(), x[b], float(alpha[b]))
            elif mode == "axpy-in-place":
                want = ops.axpy(old[b].clone(), x[b], float(alpha[b]))
            elif mode == "scale":
                want = ops.scale(x[b], float(alpha[b]))
            else:
                want = x[b]
            assert torch.equal(out[b], want), (mode, b)
        assert gaps_untouched(obase, before, n, used), mode


@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("listed", LISTS)
def test_pair_batch_equals_the_single_run_s_launches(n, listed, dtype):
    """y = g - r, s = stp d and the store of both, as `LbfgsVectors.sub_into`, `scale_into` and `store_pair` make them."""
    gen = torch.Generator().manual_seed(n + 4)
    (wbase, w), (_, g), (rbase, r), (dbase, d) = (padded(gen, inner, n, dtype) for inner in ((ROWS,), (), (), ()))
    stp = torch.tensor([1.0, 0.37, 2.5, 1.0, 0.01], dtype=dtype).cuda()
    slots = (0, 1, 2, -1, -1)
    used = list(range(NB)) if listed is None else listed
    wants = []
    for b in used:
        y = ops.scale(r[b], -1.0)
        ops.axpy(y, g[b], 1.0)
        s = ops.scale(d[b], float(stp[b])) if float(stp[b]) != 1.0 else d[b].clone()
        wants.append((y, s))
    before = [t.clone() for t in (wbase, rbase, dbase)]
    wold = w.clone()
    ops.lbfgs_pair_batch(g, r, d, w, stp, torch.tensor(slots, dtype=torch.int32).cuda(), member_list(listed))
    for b, (y, s) in zip(used, wants):
        assert torch.equal(r[b], y) and torch.equal(d[b], s), b
        for row in range(ROWS):
            want = s if row == 2 * slots[b] else y if row == 2 * slots[b] + 1 and slots[b] >= 0 else wold[b, row]
            assert torch.equal(w[b, row], want), (b, row)
    assert gaps_untouched(rbase, before[1], n, used) and gaps_untouched(dbase, before[2], n, used)
    assert gaps_untouched(wbase, before[0], ROWS * n, used)


@pytest.mark.parametrize("dtype", TDTYPES)
@pytest.mark.parametrize("shape", [(64,), (7,), (16, 16), (12, 18), (8, 8, 8), (4, 6, 10)],
                         ids=lambda s: "x".join(str(k) for k in s))
def test_poisson_adjoint_batch_equals_poisson_adjoint_per_member(shape, dtype):
    gen = torch.Generator().manual_seed(len(shape))
    cells = int(np.prod(shape))
    pad = 0 if (cells * (8 if dtype == torch.float64 else 4)) % 16 else (2 if dtype == torch.float64 else 4)
    if pad == 0:  # (members of an odd number of cells cannot lie 16 bytes apart unpadded: pad them up to it)
        pad = [p for p in range(1, 5) if ((cells + p) * (8 if dtype == torch.float64 else 4)) % 16 == 0][0]
    strides = [int(np.prod(shape[k + 1:])) for k in range(len(shape))]

    def members():
        base = torch.randn(NB * (cells + pad), generator=gen, dtype=torch.float64).to(dtype).cuda()
        return base, base.as_strided((NB,) + tuple(shape), [cells + pad] + strides)

    (_, fu), (gbase, out) = members(), members()
    h2 = [0.25, 0.5, 1.5][:len(shape)]
    before = gbase.clone()
    ops.poisson_adjoint_batch(fu, h2, 2.0 / cells, out)
    for b in range(NB):
        assert torch.equal(out[b], ops.poisson_adjoint(fu[b].contiguous(), h2, 2.0 / cells)), b
    keep = torch.ones(cells + pad, dtype=torch.bool)
    keep[:cells] = False
    keep = keep.repeat(NB).cuda()
    assert torch.equal(gbase[keep], before[keep])


# ------------------------------------------------------------------------------------- ensembles against single runs
def numbers(pinfo):
    value = lambda t: float(np.array(t))
    return value(pinfo["loss"]), [value(t) for t in pinfo["terms"]], [value(t) for t in pinfo["norms"]], list(pinfo["names"])


def lbfgs_args(epochs=6, m=3, **more):
    return argparse.Namespace(optimizer="lbfgsb", epochs=epochs, epoch_start=0, lr=0.01, bfgs_m=m, **more)


def single_runs(build, members, args):
    """Every member's own `optimize_grad(args, "lbfgsb", ...)`: [(reports, x, (nit, evals, task, warnflag))]."""
    results = []
    for b in members:
        problem, state = build(b)
        seen = []
        try:
            arrays, info = odil.util.optimize_grad(argparse.Namespace(**vars(args)), "lbfgsb", problem, state,
                                                   lambda state, epoch, pinfo, seen=seen: seen.append((epoch,) + numbers(pinfo)))
        except EarlyStopError as stop:
            info = stop.optinfo
        arrays = problem.domain.arrays_from_state(state)
        results.append((seen, [a.clone() for a in arrays], (info.epochs, info.evals, info.task, info.warnflag)))
    return results


def ensemble_run(build, members, args, form, callback=True):
    built = [build(b) for b in members]
    problems, states = [p for p, _ in built], [s for _, s in built]
    seen = [[] for _ in members]

    def report(member, state, epoch, pinfo):
        assert state is states[member]
        seen[member].append((epoch,) + numbers(pinfo))

    arrays, info = odil.util.optimize_ensemble(args, problems, states, report if callback else None, form=form)
    return arrays, info, seen, problems, states


def assert_equal_single(run, singles):
    arrays, info, seen, problems, states = run
    assert len(arrays) == len(singles)
    for j, (ref_seen, x, (nit, evals, task, warnflag)) in enumerate(singles):
        assert seen[j] == ref_seen, ("reports of member", j, seen[j], ref_seen)
        assert (int(info.nits[j]), int(info.evals[j]), info.tasks[j], int(info.warnflags[j])) == (nit, evals, task, warnflag), j
        final = problems[j].domain.arrays_from_state(states[j])
        for name, got in (("x", arrays[j]), ("state", final)):
            assert len(got) == len(x)
            for lvl, (p, q) in enumerate(zip(got, x)):
                assert p.shape == q.shape and torch.equal(p, q), (j, name, lvl, float((p - q).abs().max()))
    assert 0 < info.rounds and info.host_reads <= 2 * info.rounds + 2


TRACED = [("2d-16-3lvl", (16, 16), 3, "launches"), ("2d-16-plain-field", (16, 16), None, "launches"),
          ("1d-64-3lvl", (64,), 3, "launches"), ("3d-8-2lvl", (8, 8, 8), 2, "volumes")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["beta0", "beta1"])
@pytest.mark.parametrize("name,cshape,nlvl,form", TRACED, ids=[t[0] for t in TRACED])
def test_traced_members_equal_their_single_runs(name, cshape, nlvl, form, beta, dtype):
    """Three members, 6 iterations, bfgs_m = 3 (the history wraps): every level, every report, the counts and the task."""
    nb = 3
    args = lbfgs_args()
    build = lambda b: make_member(cshape, nlvl, dtype, b, nb, beta=beta)
    singles = single_runs(build, range(nb), args)
    run = ensemble_run(build, range(nb), args, form)
    assert run[1].route == "traced" and run[1].form == form
    assert_equal_single(run, singles)
    assert not torch.equal(run[0][0][0], run[0][1][0])
    assert max(s[2][0] for s in singles) > 3  # (more iterations than pairs the memory holds)


def _poisson():
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    return poisson


def poisson_member(spec, dtype, b):
    """Member b of a sweep over an examples/poisson problem: its own right-hand side and initial guess on every level."""
    poisson = _poisson()
    args = poisson.parse_args((spec + " --double {}".format(int(dtype == np.float64))).split())
    problem, state = poisson.make_problem(args)
    problem.extra.rhs = problem.extra.rhs * (1.0 + 0.25 * b)
    gen = torch.Generator().manual_seed(100 + b)
    domain = problem.domain
    arrays = [(0.05 * torch.randn(tuple(a.shape), generator=gen, dtype=torch.float64)).to(a.dtype).to(a.device)
              for a in domain.arrays_from_state(state)]
    domain.arrays_to_state(arrays, state)
    return problem, state


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spec,form,kind", [("--ndim 2 --N 16", "launches", "PoissonLaunchEnsemble"),
                                            ("--ndim 3 --N 8", "volumes", "PoissonVolumeEnsemble")], ids=["2d-16", "3d-8"])
def test_poisson_members_equal_their_single_runs(spec, form, kind, dtype):
    nb = 3
    args = lbfgs_args()
    build = lambda b: poisson_member(spec, dtype, b)
    singles = single_runs(build, range(nb), args)
    for asked in (form, "auto"):
        run = ensemble_run(build, range(nb), args, asked)
        assert run[1].route == "poisson" and run[1].form == form and type(run[1].ensemble).__name__ == kind
        assert_equal_single(run, singles)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_member_that_converges_early_retires_and_reports_like_its_single_run(dtype):
    """bfgs_pgtol = max |g| of member 0 after three iterations: its single run converges there (EarlyStopError) while
    the others go on; the ensemble reports the same task, counts and iterates per member, and calls back at the cadence
    `next_active` names."""
    nb = 3
    build = lambda b: make_member((16, 16), 3, dtype, b, nb, beta=0.0)
    problem, state = build(0)
    odil.util.optimize_grad(lbfgs_args(epochs=3), "lbfgsb", problem, state)
    gmax = max(float(g.abs().max()) for g in problem.eval_loss_grad_device(state)[1])
    args = lbfgs_args(epochs=8, bfgs_pgtol=gmax, bfgs_maxls=20)
    singles = single_runs(build, range(nb), args)
    assert singles[0][2][0] <= 3 and singles[0][2][2].startswith("CONVERGENCE: NORM"), [s[2] for s in singles]
    run = ensemble_run(build, range(nb), args, "launches")
    assert_equal_single(run, singles)
    # every second iteration only
    built = [build(b) for b in range(nb)]
    seen = [[] for _ in range(nb)]

    def report(member, state, epoch, pinfo):
        seen[member].append((epoch,) + numbers(pinfo))

    report.next_active = lambda epoch: (epoch // 2 + 1) * 2
    odil.util.optimize_ensemble(args, [p for p, _ in built], [s for _, s in built], report, form="launches")
    for b in range(nb):
        assert seen[b] == [r for r in singles[b][0] if r[0] % 2 == 0], b


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_member_equals_member_zero_of_five(dtype):
    nb = 5
    args = lbfgs_args()
    build = lambda b: make_member((16, 16), 3, dtype, b, nb, beta=1.0)
    five = ensemble_run(build, range(nb), args, "launches")
    one = ensemble_run(build, [0], args, "launches")
    assert all(torch.equal(p, q) for p, q in zip(one[0][0], five[0][0])) and one[2][0] == five[2][0]
    assert (int(one[1].nits[0]), int(one[1].evals[0]), one[1].tasks[0]) == (int(five[1].nits[0]), int(five[1].evals[0]), five[1].tasks[0])


def test_library_calls_per_round_do_not_grow_with_the_members(monkeypatch):
    """The same library calls, in the same order, for B = 2 and B = 6 identical Poisson members."""
    from odil_amd import _lib

    calls = []
    for nb in (2, 6):
        built = [poisson_member("--ndim 2 --N 16", np.float64, 0) for _ in range(nb)]
        called, real = [], _lib.call

        def counting(name, *args, called=called, real=real, **kwargs):
            called.append(name)
            return real(name, *args, **kwargs)

        with monkeypatch.context() as patch:
            patch.setattr(ops, "call", counting)
            _, info = odil.util.optimize_ensemble(lbfgs_args(), [p for p, _ in built], [s for _, s in built], form="launches")
        assert info.rounds >= 6
        # (ahead of the rounds: the probes of `fused.detect`, member by member; the first round begins with the synthesis)
        assert not [name for name in called[:called.index("mg_synth")] if name.startswith("lbfgs_") or "batch" in name]
        calls.append((info.rounds, info.host_reads, called[called.index("mg_synth"):]))
    assert calls[0] == calls[1]
    per_round = [name for name in calls[0][2] if name.startswith("lbfgs_") or name == "poisson_adjoint_batch"]
    assert per_round.count("poisson_adjoint_batch") == calls[0][0] and len(per_round) <= 12 * calls[0][0] + 12


def test_refusals_before_any_state_changes():
    args = lbfgs_args()
    built = [make_member((16, 16), 3, np.float64, b, 2) for b in range(2)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    before = [[a.clone() for a in p.domain.arrays_from_state(s)] for p, s in built]
    for kwargs, match in ((dict(), "form 'workgroup'"), (dict(form="launches", lrs=[0.1, 0.1]), "`lrs` are Adam's")):
        with pytest.raises(ValueError, match=match):
            odil.util.optimize_ensemble(args, problems, states, **kwargs)
    with pytest.raises(ValueError, match="bfgs_m = 65"):
        odil.util.optimize_ensemble(lbfgs_args(m=65), problems, states, form="launches")
    for (p, s), old in zip(built, before):
        assert all(torch.equal(a, b) for a, b in zip(p.domain.arrays_from_state(s), old))
