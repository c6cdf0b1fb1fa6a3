"""NumPy restatement (TEST INFRASTRUCTURE) of what one workgroup of odil_stencil_solve_krylov_batch does with its member:
stationary V(2, 2) cycles of tests/stencil_gmg_np.py (`hierarchy_axes`, `vcycle_axes`) under the kernel's decision before
every cycle, and -- once the hand-over rule fires -- GCR(m) around the same cycle with the algebra of
`gmg.PoissonGMG.solve_krylov`.  A MODEL of the algorithm, not of the kernel's arithmetic: it starts from zero (the kernel by
nested iteration), smooths with `chebyshev_weights` (the kernel with `jacobi_weights`) and has no second cycle on level 1 in
3-D.  tests/test_newton_ensemble_krylov_host.py asserts in it the facts the GPU cases rest on."""

import numpy as np
import stencil_gmg_np as sg
from oracle import odil_np as onp

CONVERGED, MAXCYCLES, STAGNATED, NONFINITE, BREAKDOWN = 0, 1, 2, 3, 4


def convection_member(shape, v, axis=0, kfun=None):
    """(coeffs, b, reference solution): the Poisson operator (kfun: div(k grad u)) plus first-order upwind convection
    - v du/dx_axis; b = A u_ref."""
    coeffs = sg.poisson_coeffs(shape) if kfun is None else sg.diffusion_coeffs(shape, kfun)
    if v:
        coeffs = sg.add_upwind_convection(coeffs, float(v), axis)
    ref = onp.poisson_ref_u(shape)
    return coeffs, sg.apply(coeffs, ref), ref


def random_diffusion(shape, rng, contrast=1.0):
    """-div(k grad u) + r u with a smooth positive conductivity (1 : 1 + contrast), face conductivities by averaging,
    zero-Dirichlet walls at half a cell: the random members of tests/test_newton_ensemble_stencil_gpu.py, restated.
    contrast 1 is what that file's anisotropic members take; at its default 19 the plain cycles of this model lose the
    1-D and 2-D members (contraction factors above 1 from the third cycle on), which makes them no benign members."""
    nd = len(shape)
    grids = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
    k = 1.0 + contrast * np.prod([np.sin(np.pi * g * rng.integers(1, 3)) ** 2 for g in grids], axis=0)
    off, diag = [], rng.uniform(0.0, 1.0, shape)
    h2 = (1.0 / max(shape)) ** 2
    for a in range(nd):
        km = 0.5 * (k + np.roll(k, 1, axis=a)) / h2
        kp = 0.5 * (k + np.roll(k, -1, axis=a)) / h2
        idx = np.arange(shape[a]).reshape([-1 if j == a else 1 for j in range(nd)])
        diag = diag + np.where(idx == 0, 2.0 * k / h2, km) + np.where(idx == shape[a] - 1, 2.0 * k / h2, kp)
        off += [-np.where(idx == 0, 0.0, km), -np.where(idx == shape[a] - 1, 0.0, kp)]
    return np.stack([diag] + off)


def benign_members(shape, nb, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([random_diffusion(shape, rng) for _ in range(nb)])


def member_coeffs(shape, v, kind):
    """[2 d + 1, *shape]: kind None -- the Poisson operator with upwind convection - v du/dx_0; RANDOM -- a member of
    `random_diffusion` (its sign turned to the Poisson operator's: negative diagonal) with the same convection.  Pure
    diffusion coarsens every axis alike on every level, convection makes axis 0 the weak one from level 1 on: a random
    diffusion member walks the levels of the convective members only with some convection of its own (v = 50: benign)."""
    if kind is None:
        return np.stack(convection_member(shape, v, 0)[0])
    assert kind == RANDOM
    coeffs = [-c for c in random_diffusion(shape, np.random.default_rng(5))]
    return np.stack(sg.add_upwind_convection(coeffs, float(v), 0) if v else coeffs)


RANDOM = "random diffusion"
# (name, shape, cycle budget, members as (v, None or RANDOM: `member_coeffs`), the hard members, the benign ones)
CASE_A = ("A", (64,), 60, [(0.0, None), (200.0, None)], [1], [0])
CASE_B = ("B", (8, 8, 8), 40, [(200.0, None), (800.0, None), (50.0, RANDOM)], [1], [2])
CASES = [CASE_A, CASE_B]


def case_arrays(case):
    """(coeffs [B, 2 d + 1, *shape], b [B, *shape]) in float64; b = A u of a ROUGH u (normal deviates).  The residual a
    working precision can reach is eps | |A| |x| | / |b|: for a smooth solution on 64 cells |b| = |A x| is ~ 1e3 times
    smaller than | |A| |x| |, which puts the float32 floor (~1e-4) above the driver's 50 eps and lets no float32 solver
    report convergence; for a rough one the two are of one size and the floor is a few eps."""
    _, shape, _, members, _, _ = case
    rng = np.random.default_rng(17)
    coeffs = np.stack([member_coeffs(shape, v, kind) for v, kind in members])
    b = np.stack([sg.apply(list(c), rng.standard_normal(shape)) for c in coeffs])
    return coeffs, b


def level_shapes(coeffs):
    return [tuple(level[0].shape) for level in sg.hierarchy_axes(coeffs)[0]]


def solve(coeffs, b, tol=1e-10, maxcycles=60, krylov="auto", m=6):
    """dict(x, niter, why, handover, history): history[0] = mean(b^2), history[1 + k] = the mean square of the residual before
    pass k; the decision order of the kernel (include/odil_hip.h)."""
    levels, halves = sg.hierarchy_axes(coeffs)
    cycle = lambda x, r: sg.vcycle_axes(levels, halves, 0, x, r)
    msq = lambda r: float(np.mean(r * r))
    tol2, bsq = tol * tol, msq(b)
    x, history, prev, k, handover = np.zeros_like(b), [bsq], bsq, 0, None
    while True:
        rsq = msq(sg.apply(coeffs, x) - b)
        history.append(rsq)
        if not np.isfinite(rsq) or not np.isfinite(bsq):
            return dict(x=x, niter=k, why=NONFINITE, handover=None, history=history)
        if rsq <= tol2 * bsq:
            return dict(x=x, niter=k, why=CONVERGED, handover=None, history=history)
        if k == maxcycles:
            return dict(x=x, niter=k, why=MAXCYCLES, handover=None, history=history)
        if krylov == "auto" and k >= 2 and rsq >= 0.25 * prev and rsq > 1e6 * tol2 * bsq:
            handover = k
            break
        if k >= 3 and rsq >= 0.98 ** 2 * prev:
            return dict(x=x, niter=k, why=STAGNATED, handover=None, history=history)
        prev = rsq
        x = cycle(x, b)
        k += 1
    rho, Z, Q = b - sg.apply(coeffs, x), [], []
    while True:
        z = cycle(np.zeros_like(b), rho)
        q = sg.apply(coeffs, z)
        betas = [float(np.vdot(qj, q)) for qj in Q]  # (classical Gram-Schmidt: all products with the un-projected q)
        for beta, zj, qj in zip(betas, Z, Q):
            q, z = q - beta * qj, z - beta * zj
        qq = float(np.vdot(q, q))
        if not qq > 0.0 or not np.isfinite(qq):
            return dict(x=x, niter=k, why=BREAKDOWN, handover=handover, history=history)
        q, z = q / np.sqrt(qq), z / np.sqrt(qq)
        a = float(np.vdot(q, rho))
        x, rho = x + a * z, rho - a * q
        Z.append(z), Q.append(q)
        k += 1
        history.append(msq(rho))
        why = None
        if not np.isfinite(history[-1]):
            why = NONFINITE
        elif history[-1] <= tol2 * bsq:  # (the recurrence says converged: the true residual decides)
            rho, Z, Q = b - sg.apply(coeffs, x), [], []
            history[-1] = msq(rho)
            why = CONVERGED if history[-1] <= tol2 * bsq else None
        if why is None and k == maxcycles:
            why = MAXCYCLES
        if why is not None:
            return dict(x=x, niter=k, why=why, handover=handover, history=history)
        if len(Z) == m:
            Z, Q = [], []
