"""Newton ensembles of variable-coefficient stencil problems on the device: the batched hierarchy set-up
(odil_stencil_var_coarsen_batch, odil_stencil_strength_batch, odil_stencil_dense_batch), gmg.EnsembleGMG.from_coeffs /
rebuild and the stencil route of util.optimize_newton_ensemble.

1  set-up bit pins: every member of a padded pack equals the single entry points (odil_stencil_var_coarsen[_axes],
   odil_max_abs_rows, the column-by-column dense matrix) bit for bit, canaries between the members stay, a member computes
   the same bits alone and inside a batch
2  EnsembleGMG.from_coeffs(pack) against [StencilGMG(pack[b])]: shapes, halve, coefficients of every level, coarsest
   inverse; rebuild in place; members that disagree are named
3  the solve launch fed by the batched set-up against single launches of ops.stencil_vcycle_tail
4  optimize_newton_ensemble on examples/diffusion members against single optimize_newton runs and a float64 dense Newton
   iteration in NumPy (a restatement of the example's operator: tests/jacobian_ref.py runs operators whose `extra` is an
   array, the example keeps its conductivities in a namespace)
5  the same with the nonlinear term beta u^3
6  float32 against the float64 reference
7  routing: all-Poisson ensembles keep their route; members with other unknowns are refused by name"""

import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT

pytestmark = pytest.mark.gpu

CANARY = 777.0
F64, F32 = torch.float64, torch.float32
CASES = [((64,), None), ((12, 20), None), ((8, 4, 16), None), ((16, 16, 16), None), ((16, 16, 16), 0)]
CASE_IDS = ["64", "12x20", "8x4x16", "16^3", "16^3-periodic"]
NMAX = 70


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


def diffusion_coeffs(shape, rng, periodic=None, scale0=1.0, contrast=19.0):
    """-div(k grad u) + r u with a smooth positive conductivity (1 : 1 + contrast), face conductivities by averaging,
    zero-Dirichlet walls at half a cell or one periodic axis, in the layout of the Jacobian's coefficient arrays (0, -e_0,
    +e_0, ...); scale0: factor on the couplings of axis 0 (an anisotropic operator)."""
    nd = len(shape)
    grids = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
    k = 1.0 + contrast * np.prod([np.sin(np.pi * g * rng.integers(1, 3)) ** 2 for g in grids], axis=0)
    off, diag = [], rng.uniform(0.0, 1.0, shape)
    for a in range(nd):
        h2 = (1.0 / max(shape)) ** 2 / (scale0 if a == 0 else 1.0)
        km = 0.5 * (k + np.roll(k, 1, axis=a)) / h2
        kp = 0.5 * (k + np.roll(k, -1, axis=a)) / h2
        idx = np.arange(shape[a]).reshape([-1 if j == a else 1 for j in range(nd)])
        if periodic != a:
            diag = diag + np.where(idx == 0, 2.0 * k / h2, km) + np.where(idx == shape[a] - 1, 2.0 * k / h2, kp)
            km, kp = np.where(idx == 0, 0.0, km), np.where(idx == shape[a] - 1, 0.0, kp)
        else:
            diag = diag + km + kp
        off += [-km, -kp]
    return np.stack([diag] + off)


def members_pack(shape, periodic, dtype, dev, nb, seed=5, scale0=None):
    """[nb, 2 d + 1, *shape]: one operator per member; scale0: per member the factor on the axis-0 couplings.  With it
    the conductivity varies 1 : 2 only: a merged axis loses a factor 4 per level against the others, so the ratios of the
    couplings are 25 and 6.25 x [1/2, 2] on the levels of the shapes below -- every member on the same side of the
    factor 2 at which `StencilGMG` begins to merge the weak axes too."""
    rng = np.random.default_rng(seed)
    arrays = [diffusion_coeffs(shape, rng, periodic, 1.0 if scale0 is None else scale0[b], 19.0 if scale0 is None else 1.0)
              for b in range(nb)]
    return torch.tensor(np.stack(arrays), dtype=dtype, device=dev)


def padded_rows(members, pad):
    """[B, need + pad]: the members' arrays at the start of the rows, canaries behind them."""
    nb = members.shape[0]
    flat = members.reshape(nb, -1)
    base = torch.full((nb, flat.shape[1] + pad), CANARY, dtype=members.dtype, device=members.device)
    base[:, :flat.shape[1]].copy_(flat)
    return base


def canaries_intact(base, need):
    return bool((base[:, need:] == CANARY).all())


HALVES = {1: [None], 2: [None, (1, 0)], 3: [None, (1, 0, 1)]}


class SingleReference:
    """What the single entry points give for the members of one (shape, periodic, dtype), member by member, computed when
    first asked for and kept."""

    def __init__(self, shape, periodic, dtype, dev):
        self.shape, self.ndim = shape, len(shape)
        self.pack = members_pack(shape, periodic, dtype, dev, NMAX)
        self.coarse_shape = tuple(n // 2 for n in shape)
        self._coarse, self._strength, self._dense = dict(), dict(), dict()

    def coarse(self, m, halve):
        from odil_amd import ops

        if (m, halve) not in self._coarse:
            self._coarse[(m, halve)] = ops.stencil_var_coarsen(self.pack[m].contiguous(), None if halve is None else list(halve))
        return self._coarse[(m, halve)]

    def strength(self, m):
        from odil_amd import ops

        if m not in self._strength:
            self._strength[m] = ops.max_abs_rows(self.pack[m, 1:].contiguous())
        return self._strength[m]

    def dense(self, m):
        """Column j = A e_j of the once-coarsened operator of member m (at most 512 unknowns), one launch per column: what
        gmg.StencilGMG.coarse_column gives `coarse_inverse`."""
        from odil_amd import ops

        if m not in self._dense:
            coeffs = self.coarse(m, None)
            n = math.prod(self.coarse_shape)
            eye = torch.eye(n, dtype=coeffs.dtype, device=coeffs.device)
            zero = torch.zeros(self.coarse_shape, dtype=coeffs.dtype, device=coeffs.device)
            cols = [(-ops.stencil_var_residual(coeffs, eye[j].view(self.coarse_shape), zero)).reshape(-1) for j in range(n)]
            self._dense[m] = torch.stack(cols, dim=1)
        return self._dense[m]


_single = dict()


def single_reference(shape, periodic, dtype, dev):
    key = (shape, periodic, dtype)
    if key not in _single:
        _single[key] = SingleReference(shape, periodic, dtype, dev)
    return _single[key]


def checked_members(nb):
    return sorted({0, 1, 2, nb // 2, nb - 1} & set(range(nb)))


# ------------------------------------------------------------------------------------------------ 1: set-up bit pins
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nb", [1, 3, NMAX])
@pytest.mark.parametrize("shape,periodic", CASES, ids=CASE_IDS)
def test_coarsen_batch_equals_single_launches(dev, shape, periodic, nb, dtype):
    from odil_amd import ops

    ref = single_reference(shape, periodic, dtype, dev)
    nd = len(shape)
    base = padded_rows(ref.pack[:nb], 7)
    need = (2 * nd + 1) * math.prod(shape)
    for halve in HALVES[nd]:
        cshape = tuple(n // 2 if (halve is None or halve[a]) else n for a, n in enumerate(shape))
        cneed = (2 * nd + 1) * math.prod(cshape)
        out = torch.full((nb, cneed + 5), CANARY, dtype=dtype, device=dev)
        ops.stencil_var_coarsen_batch(base, shape, halve, out=out)
        assert canaries_intact(out, cneed) and canaries_intact(base, need), "padding between members was written"
        for m in range(nb):
            assert torch.equal(out[m, :cneed], ref.coarse(m, halve).reshape(-1)), (halve, m)
        fresh = ops.stencil_var_coarsen_batch(ref.pack[:nb].reshape(nb, -1), shape, halve)  # (no padding, own output)
        assert torch.equal(fresh, out[:, :cneed])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nb", [1, 3, NMAX])
@pytest.mark.parametrize("shape,periodic", CASES, ids=CASE_IDS)
def test_strength_batch_equals_max_abs_rows(dev, shape, periodic, nb, dtype):
    from odil_amd import ops

    ref = single_reference(shape, periodic, dtype, dev)
    nd = len(shape)
    base = padded_rows(ref.pack[:nb], 7)
    out = torch.full((nb + 1, 2 * nd), CANARY, dtype=dtype, device=dev)
    ops.stencil_strength_batch(base, shape, out=out[:nb])
    assert bool((out[nb] == CANARY).all()) and canaries_intact(base, (2 * nd + 1) * math.prod(shape))
    for m in range(nb):
        assert torch.equal(out[m], ref.strength(m)), (m, out[m], ref.strength(m))
    # a canary behind a member is not part of it: a padding LARGER than every coefficient must not show
    base[:, (2 * nd + 1) * math.prod(shape):] = 1e30
    assert torch.equal(ops.stencil_strength_batch(base, shape), out[:nb])


def test_strength_batch_propagates_nan(dev):
    from odil_amd import ops

    shape = (12, 20)
    pack = single_reference(shape, None, F64, dev).pack[:3].clone()
    pack[1, 3, 5, 7] = float("nan")
    got = ops.stencil_strength_batch(pack.reshape(3, -1), shape).cpu().numpy()
    want = np.stack([ops.max_abs_rows(pack[m, 1:].contiguous()).cpu().numpy() for m in range(3)])
    assert np.isnan(got[1, 2]) and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[[0, 2]], want[[0, 2]])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("nb", [1, 3, NMAX])
@pytest.mark.parametrize("shape,periodic", CASES, ids=CASE_IDS)
def test_dense_batch_equals_the_columns(dev, shape, periodic, nb, dtype):
    """On the once-coarsened operators ((32,), (6, 10), (4, 2, 8) -- an axis of extent 2, where -e and +e meet in one entry
    -- and 8^3 = 512 unknowns, the limit, with and without the periodic wrap)."""
    from odil_amd import ops

    ref = single_reference(shape, periodic, dtype, dev)
    cshape, n = ref.coarse_shape, math.prod(ref.coarse_shape)
    coarse = torch.stack([ref.coarse(m, None) for m in range(nb)])
    base = padded_rows(coarse, 3)
    out = torch.full((nb + 1, n, n), CANARY, dtype=dtype, device=dev)
    ops.stencil_dense_batch(base, cshape, out=out[:nb])
    assert bool((out[nb] == CANARY).all()) and canaries_intact(base, coarse[0].numel())
    assert not bool((out[:nb] == CANARY).any())
    for m in checked_members(nb):
        assert torch.equal(out[m], ref.dense(m)), m
    if nb == 3:  # (a member alone, on its own arrays)
        for m in range(nb):
            assert torch.equal(ops.stencil_dense_batch(coarse[m].reshape(1, -1), cshape)[0], out[m])


def test_a_member_computes_the_same_alone_and_inside_a_batch(dev):
    from odil_amd import ops

    shape, nb = (16, 16, 16), 5
    pack = single_reference(shape, 0, F64, dev).pack[:nb].reshape(nb, -1)
    for halve in HALVES[3]:
        batch = ops.stencil_var_coarsen_batch(pack, shape, halve)
        for m in range(nb):
            assert torch.equal(ops.stencil_var_coarsen_batch(pack[m:m + 1].clone(), shape, halve)[0], batch[m])
    batch = ops.stencil_strength_batch(pack, shape)
    for m in range(nb):
        assert torch.equal(ops.stencil_strength_batch(pack[m:m + 1].clone(), shape)[0], batch[m])


# --------------------------------------------------------------------------------------------------- 2: hierarchy pin
def assert_same_hierarchy(ens, singles):
    for b, h in enumerate(singles):
        assert [tuple(s) for s in h.shapes] == [tuple(s) for s in ens.shapes], (b, h.shapes, ens.shapes)
        assert list(h.locs) == list(ens.locs) and (h.nu1, h.nu2) == (ens.nu1, ens.nu2)
        for lvl in range(len(ens.shapes)):
            assert torch.equal(ens.level(lvl)[b], h.coeffs[lvl].reshape(-1)), (b, lvl)
        assert torch.equal(ens.inv[b], h.coarse_inverse()), b
    assert ens.halve == [[c == "c" for c in loc] for loc in ens.locs]


HIERARCHIES = [((16, 16), None, None), ((12, 20), None, None), ((16, 16, 16), 0, None), ((8, 16), None, 100.0),
               ((8, 4, 16), None, 100.0)]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,periodic,scale0", HIERARCHIES, ids=["16^2", "12x20", "16^3-periodic", "8x16-aniso", "8x4x16-aniso"])
def test_from_coeffs_equals_stencil_gmg(dev, shape, periodic, scale0, dtype):
    from odil_amd import gmg

    nb = 4
    pack = members_pack(shape, periodic, dtype, dev, nb, seed=7, scale0=None if scale0 is None else [scale0] * nb)
    ens = gmg.EnsembleGMG.from_coeffs(pack)
    singles = [gmg.StencilGMG(pack[b].contiguous()) for b in range(nb)]
    assert_same_hierarchy(ens, singles)
    assert ens.coeffs.dim() == 2 and ens.inv.dim() == 3 and ens.nbatch == nb and torch.equal(ens.fine, pack)
    if scale0 is not None:
        assert ens.halve[0][0] and not all(ens.halve[0]), ens.halve  # (semi-coarsening: axis 0 first)
    # rebuild: the bits of a fresh object in the same buffers
    buffers = [t.data_ptr() for t in (ens.coeffs, ens.inv, ens.work, ens._dense, ens._strength)]
    launch = ens._launch
    other = members_pack(shape, periodic, dtype, dev, nb, seed=8, scale0=None if scale0 is None else [scale0] * nb)
    ens.rebuild(other)
    assert buffers == [t.data_ptr() for t in (ens.coeffs, ens.inv, ens.work, ens._dense, ens._strength)]
    assert ens._launch is launch
    assert_same_hierarchy(ens, [gmg.StencilGMG(other[b].contiguous()) for b in range(nb)])
    fresh = gmg.EnsembleGMG.from_coeffs(other)
    assert torch.equal(fresh.coeffs, ens.coeffs) and torch.equal(fresh.inv, ens.inv) and fresh.shapes == ens.shapes


def test_rebuild_plans_anew_when_all_members_change_their_axes(dev):
    from odil_amd import gmg

    shape, nb = (16, 16), 3
    ens = gmg.EnsembleGMG.from_coeffs(members_pack(shape, None, F64, dev, nb, seed=7))
    assert all(all(halve) for halve in ens.halve)
    # (x 400: the ratios 100, 25 and 6.25 x [1/2, 2] on (8, 16), (4, 16) and (2, 16), where axis 0 cannot be merged again)
    aniso = members_pack(shape, None, F64, dev, nb, seed=7, scale0=[400.0] * nb)
    ens.rebuild(aniso)
    assert ens.shapes == [(16, 16), (8, 16), (4, 16), (2, 16)]
    assert_same_hierarchy(ens, [gmg.StencilGMG(aniso[b].contiguous()) for b in range(nb)])
    assert not all(ens.halve[0])


def test_members_that_disagree_are_named(dev):
    from odil_amd import gmg

    shape, nb = (16, 16), 3
    pack = members_pack(shape, None, F64, dev, nb, seed=7, scale0=[1.0, 100.0, 1.0])
    with pytest.raises(ValueError, match="member 1 .*level 0"):
        gmg.EnsembleGMG.from_coeffs(pack)
    ens = gmg.EnsembleGMG.from_coeffs(members_pack(shape, None, F64, dev, nb, seed=7))
    with pytest.raises(ValueError, match="member 1 .*level 0"):
        ens.rebuild(pack)


def test_from_coeffs_reports_the_limits(dev):
    from odil_amd import gmg

    with pytest.raises(ValueError, match="cells are above the limit"):
        gmg.EnsembleGMG.from_coeffs(torch.zeros((1, 5, 256, 256), dtype=F64, device=dev))
    with pytest.raises(ValueError, match="coarsest level of at most 512"):  # 100 -> 50 -> 25: 625 unknowns
        gmg.EnsembleGMG.from_coeffs(members_pack((100, 100), None, F64, dev, 2))


# ------------------------------------------------------------------------------------------------------- 3: solve pin
def random_members(nb, shape, dtype, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((nb,) + tuple(shape), generator=gen, dtype=torch.float64).to(dtype).to(dev)


def single_tail_launches(ens, member, b, x0, ks=(0, 1, 3)):
    """{(start, k): iterate} of ONE member by single launches of the one-workgroup cycle on its arrays alone."""
    from odil_amd import ops

    work = torch.empty(3 * sum(math.prod(s) for s in ens.shapes), dtype=ens.dtype, device=b.device)
    launch = ops.stencil_vcycle_tail_plan(ens.coeffs[member].contiguous(), ens.shapes, ens.halve, work,
                                          ens.inv[member].contiguous(), ens.wpre, ens.wpost)
    b = b.contiguous()
    out = dict()
    for start in (0, 1, 2):
        if start == 0:
            x, zero = torch.zeros_like(b), True
        elif start == 1:
            x, zero = x0.clone(), False
        else:
            x, zero = launch(None, b, torch.empty_like(b), fmg=True), False
        for k in range(max(ks) + 1):
            if k in ks:
                out[(start, k)] = x.clone()
            x = launch(None if zero else x, b, torch.empty_like(b))
            zero = False
    return out


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,periodic,scale0", [((16, 16), None, None), ((16, 16, 16), 0, None), ((8, 16), None, 100.0)],
                         ids=["16^2", "16^3-periodic", "8x16-aniso"])
def test_solve_after_batched_setup_equals_single_tail_launches(dev, shape, periodic, scale0, dtype):
    from odil_amd import gmg

    nb = 3
    ens = gmg.EnsembleGMG.from_coeffs(members_pack(shape, periodic, dtype, dev, nb, seed=9,
                                                   scale0=None if scale0 is None else [scale0] * nb))
    b = random_members(nb, shape, dtype, dev, 21)
    x0 = random_members(nb, shape, dtype, dev, 22)
    refs = [single_tail_launches(ens, m, b[m], x0[m]) for m in range(nb)]
    for start in (0, 1, 2):
        for k in (0, 1, 3):
            x = x0.clone()
            ens.solve(b, x, tol=0.0, maxcycles=k, start=start)
            for m in range(nb):
                assert torch.equal(x[m], refs[m][(start, k)]), (start, k, m)
            assert (ens.outcome[:, 0] == k).all() and (ens.outcome[:, 1] == 1).all(), (start, k, ens.outcome)


# ------------------------------------------------------------------------------------------------------ 4-6: public API
def _api():
    sys.path.insert(0, os.path.join(ROOT, "examples", "diffusion"))
    import ensemble

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    return odil, ensemble


def _member(ensemble, spec, b, nb, epochs):
    """Member b of a sweep over examples/diffusion: its own conductivity amplitude (ensemble.make_member), right-hand side
    and initial guess."""
    args = ensemble.parse_args((spec + " --members {}".format(nb)).split())
    args.epoch_start, args.epochs = 0, epochs
    problem, state = ensemble.make_member(args, b)
    domain = problem.domain
    gen = torch.Generator().manual_seed(300 + b)
    rhs = problem.extra.rhs
    noise = torch.randn(tuple(rhs.shape), generator=gen, dtype=F64).to(rhs.dtype).to(rhs.device)
    problem.extra.rhs = rhs * (1.0 + 0.25 * b) + 0.1 * noise
    (a,) = domain.arrays_from_state(state)
    domain.arrays_to_state([0.05 * torch.randn(tuple(a.shape), generator=gen, dtype=F64).to(a.dtype).to(a.device)], state)
    return args, problem, state


def np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


class DenseMember:
    """The member's operator f(u) = sum_i [k_i+ (g_i+ - u) - k_i- (u - g_i-)] / h_i^2 - beta u^3 - rhs (wall ghosts by
    quadratic extrapolation through 0 at the wall) and its Jacobian as a dense matrix, in NumPy float64."""

    def __init__(self, problem, state):
        extra, domain = problem.extra, problem.domain
        self.kfaces = [(np64(km), np64(kp)) for km, kp in extra.kfaces]
        self.rhs, self.u0 = np64(extra.rhs), np64(state.fields["u"].array)
        self.h = [float(domain.step_by_dim(i)) for i in range(domain.ndim)]
        self.beta, self.shape = float(extra.beta), self.u0.shape
        n = self.u0.size
        eye = np.eye(n).reshape((n,) + self.shape)
        self.linear = np.stack([self.flux(eye[j]).reshape(-1) for j in range(n)], axis=1)  # column j = L e_j

    def flux(self, u):
        total = np.zeros_like(u)
        for i, (km, kp) in enumerate(self.kfaces):
            n = u.shape[i]
            idx = np.arange(n).reshape([-1 if j == i else 1 for j in range(u.ndim)])
            qm, qp = np.roll(u, 1, i), np.roll(u, -1, i)
            gm = np.where(idx == 0, (qp - 6 * u) / 3, qm)
            gp = np.where(idx == n - 1, (qm - 6 * u) / 3, qp)
            total = total + (kp * (gp - u) - km * (u - gm)) / self.h[i] ** 2
        return total

    def f(self, u):
        return self.flux(u) - self.beta * u ** 3 - self.rhs

    def jacobian(self, u):
        return self.linear - np.diag(3 * self.beta * u.reshape(-1) ** 2)

    def newton(self, epochs):
        """(iterates u_0 .. u_epochs, |d| of the first step, the largest cond(J) on the way)."""
        us, first, cond = [self.u0], None, 0.0
        for _ in range(epochs):
            J = self.jacobian(us[-1])
            d = np.linalg.solve(J, self.f(us[-1]).reshape(-1)).reshape(self.shape)
            first = np.linalg.norm(d) if first is None else first
            cond = max(cond, np.linalg.cond(J))
            us.append(us[-1] - d)
        return us, first, cond


def _run_ensemble(odil, ensemble, spec, nb, epochs):
    built = [_member(ensemble, spec, b, nb, epochs) for b in range(nb)]
    args, problems, states = built[0][0], [p for _, p, _ in built], [s for _, _, s in built]
    dense = [DenseMember(p, s) for p, s in zip(problems, states)]
    seen = [[] for _ in range(nb)]

    def callback(member, state, epoch, pinfo):
        assert state is states[member]
        seen[member].append((epoch, float(np.array(pinfo["loss"])), pinfo.get("linsolver"), np64(state.fields["u"].array)))

    arrays, info = odil.util.optimize_newton_ensemble(args, problems, states, callback)
    return args, problems, states, dense, seen, arrays, info


def _check_against_references(odil, ensemble, spec, nb, epochs, tol=1e-10):
    args, problems, states, dense, seen, arrays, info = _run_ensemble(odil, ensemble, spec, nb, epochs)
    cshape = tuple(problems[0].domain.cshape)
    assert info.route == "stencil" and "variable coefficients" in info.solver.method
    assert len(arrays) == nb and info.epochs == epochs and info.cycles.shape == (nb, epochs) and info.residuals.shape == (nb, epochs)
    base = states[0].fields["u"].array.untyped_storage().data_ptr()
    for b in range(nb):
        assert [e for e, _, _, _ in seen[b]] == list(range(epochs + 1))
        assert seen[b][0][2] is None
        for _, _, st, _ in seen[b][1:]:
            assert st["converged"] and st["method"] == info.solver.method, (b, st)
        assert info.cycles[b, epochs - 1] == seen[b][epochs][2]["niter"] >= 1
        field = states[b].fields["u"].array
        assert field.untyped_storage().data_ptr() == base and field.storage_offset() == b * math.prod(cshape)
        assert arrays[b][0].data_ptr() == field.data_ptr()
        us, dnorm, cond = dense[b].newton(epochs)
        bound = 2 * cond * tol * dnorm
        got = np64(field)
        sargs, sproblem, sstate = _member(ensemble, spec, b, nb, epochs)
        odil.util.optimize_newton(sargs, sproblem, sstate)
        alone = np64(sstate.fields["u"].array)
        moved = np.linalg.norm(seen[b][-1][3] - seen[b][-2][3])
        print("api", spec, b, "cond", cond, "vs dense Newton", np.linalg.norm(got - us[-1]), "vs optimize_newton",
              np.linalg.norm(got - alone), "last step moved", moved, "bound", bound)
        assert np.linalg.norm(got - us[-1]) <= bound and np.linalg.norm(got - alone) <= bound
        assert moved <= bound or dense[b].beta  # (a linear member is at its solution after one step)
    return seen, dense


SPECS = ["--ndim 1 --N 64", "--ndim 2 --N 16", "--ndim 3 --N 8"]


@pytest.mark.parametrize("kind", ["smooth", "jump"])
@pytest.mark.parametrize("spec", SPECS, ids=["1d-64", "2d-16", "3d-8"])
def test_optimize_newton_ensemble_linear_float64(dev, spec, kind):
    """Every comparison within 2 cond(J) tol |d|: a relative residual of tol leaves |A^-1| |r| <= cond(J) tol |d| of the
    exact step (the bound of tests/test_newton_ensemble_gpu.py::test_optimize_newton_ensemble_float64, with the member's own
    dense Jacobian); the second step of a linear member moves it by no more."""
    odil, ensemble = _api()
    _check_against_references(odil, ensemble, spec + " --kind {} --linsolver multigrid".format(kind), 5, 2)


def test_optimize_newton_ensemble_nonlinear_float64(dev):
    """beta = 1: the hierarchies are rebuilt every step.  Losses fall from step to step down to the rounding floor of the
    residual evaluation: ~8 d operations per cell on terms of size |c0| |u|, each rounded to eps."""
    odil, ensemble = _api()
    epochs = 4
    seen, dense = _check_against_references(odil, ensemble, "--ndim 2 --N 16 --kind smooth --beta 1 --linsolver multigrid", 5, epochs)
    for b in range(5):
        assert [e for e, _, _, _ in seen[b]] == [0, 1, 2, 3, 4]
        losses = [loss for _, loss, _, _ in seen[b]]
        cmax = np.abs(np.diag(dense[b].jacobian(seen[b][-1][3]))).max()
        floor = (8 * 2 * np.finfo(np.float64).eps * cmax * np.abs(seen[b][-1][3]).max()) ** 2
        print("nonlinear", b, "losses", losses, "floor", floor)
        assert losses[1] < losses[0]
        for before, after in zip(losses, losses[1:]):
            assert after < before or before <= floor, (b, losses, floor)


def test_optimize_newton_ensemble_float32(dev):
    """Both routes stop at the float32 rounding floor: the ensemble's error against the float64 reference is at most 4 x
    that of the member's single float32 optimize_newton run (operation order)."""
    odil, ensemble = _api()
    nb, spec = 5, "--ndim 2 --N 16 --kind smooth --linsolver multigrid --double 0"
    args, problems, states, dense, seen, arrays, info = _run_ensemble(odil, ensemble, spec, nb, 2)
    assert info.route == "stencil"
    for b in range(nb):
        assert states[b].fields["u"].array.dtype == F32
        want = dense[b].newton(2)[0][-1]
        sargs, sproblem, sstate = _member(ensemble, spec, b, nb, 2)
        odil.util.optimize_newton(sargs, sproblem, sstate)
        scale = np.linalg.norm(want)
        err = np.linalg.norm(np64(states[b].fields["u"].array) - want) / scale
        alone = np.linalg.norm(np64(sstate.fields["u"].array) - want) / scale
        print("api float32", b, "ensemble error", err, "optimize_newton error", alone)
        assert err <= 4 * alone, (b, err, alone)


# ---------------------------------------------------------------------------------------------------------- 7: routing
def test_all_poisson_ensembles_keep_their_route(dev):
    sys.path.insert(0, os.path.join(ROOT, "examples", "poisson"))
    import poisson

    import odil_amd as odil

    odil.util.set_log_file(open(os.devnull, "w"))
    built = []
    for b in range(3):
        args = poisson.parse_args("--multigrid 0 --optimizer newton --ndim 2 --N 16 --linsolver multigrid".split())
        args.epoch_start, args.epochs = 0, 1
        problem, state = poisson.make_problem(args)
        problem.extra.rhs = problem.extra.rhs * (1.0 + 0.25 * b)
        built.append((args, problem, state))
    seen = []
    arrays, info = odil.util.optimize_newton_ensemble(built[0][0], [p for _, p, _ in built], [s for _, _, s in built],
                                                      lambda member, state, epoch, pinfo: seen.append(pinfo.get("linsolver")))
    assert info.route == "poisson" and info.solver.method == "gmg-vcycle, one workgroup per member"
    assert [st["method"] for st in seen if st is not None] == ["gmg-vcycle, one workgroup per member"] * 3


def two_field_member(odil, args):
    domain = odil.Domain(cshape=[16, 16], dimnames=["x", "y"], multigrid=False, dtype=np.float64)
    state = domain.init_state(odil.State(fields={"u": None, "v": None}))

    def operator(ctx):
        return [ctx.field("u") - ctx.field("v"), ctx.field("u") + ctx.field("v") - 1]

    return odil.Problem(operator, domain, argparse.Namespace(args=args)), state


@pytest.mark.parametrize("which,reason", [("multigrid", "MultigridField .*no multigrid decomposition"),
                                          ("two-field", "2 unknown fields")])
def test_members_with_other_unknowns_are_refused_by_name(dev, which, reason):
    odil, ensemble = _api()
    spec = "--ndim 2 --N 16 --kind smooth --linsolver multigrid"
    built = [_member(ensemble, spec, b, 3, 2) for b in range(3)]
    args, problems, states = built[0][0], [p for _, p, _ in built], [s for _, _, s in built]
    if which == "multigrid":
        margs = ensemble.parse_args((spec + " --multigrid 1 --members 3").split())
        problems[1], states[1] = ensemble.make_member(margs, 1)
    else:
        problems[1], states[1] = two_field_member(odil, args)
    before = [(s.fields["u"].array.data_ptr(), s.fields["u"].array.clone()) for s in (states[0], states[2])]
    with pytest.raises(ValueError, match="optimize_newton_ensemble: member 1: .*{}".format(reason)):
        odil.util.optimize_newton_ensemble(args, problems, states)
    for s, (p, a) in zip((states[0], states[2]), before):
        assert s.fields["u"].array.data_ptr() == p and torch.equal(s.fields["u"].array, a)
