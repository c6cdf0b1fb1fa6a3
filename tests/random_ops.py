"""Random straight-line stencil operators shared by the GPU parity test of the generated kernels
(tests/test_workloads_gpu.py), the CPU check of the symbolic gradient expressions (tests/test_stencil_grad_host.py), the
tests of the generated Jacobian kernel (tests/test_jacobian_kernel_host.py, tests/test_jacobian_kernel_gpu.py) and the 1-D,
2-D and 3-D cases that run the folded copies of the generated kernels and the staggered and 4-D cases beside them
(tests/traced_cases.py)."""

import numpy as np

COEFF = (0.7, -0.4, 1.3)  # the values of the `Array` named "coeff"; with params=False the constants that stand for it


def random_operator(seed, params=True, ndim=2, out_locs=None, locs=None):
    """A random straight-line program over shifted reads of two fields, index masks, constants and
    the elementwise vocabulary of `mod` (smooth where it has to be: divisors and log / sqrt arguments
    are kept away from zero).

    params=False: the same program from the same random stream, the three values of the `Array` "coeff" replaced by the
    constants `COEFF` (no `ctx.field("coeff")`: a state of plain `Field`s, what `Problem.linearize` takes).
    ndim: the grid's dimensions (1 .. 4): shifts with that many components, indices and points of that many axes, rolls
    over all axes, rows imposed on axis 0 (`ctx.extra`: an array of the shape of one such row, i.e. of the output grid
    without axis 0).  The default call is the two-dimensional program with the parameter array.
    out_locs: the grids of the outputs, a list of location strings such as ["nc", "cc"] (default: the cell grid).  Per entry
    one group of outputs on that grid, all groups from the same plan: indices, points and EVERY field read are taken at the
    group's location, so a field that lives elsewhere is padded ('c' -> 'n') or trimmed ('n' -> 'c') by the read.  With
    several entries the names of the outputs carry the group ("g1f0") and the operator returns outputs of several shapes.
    locs: the locations of the fields "a" and "b" (default: cell centres).  Where any of them differs from any output grid
    the program CONVERTS, and the steps the tracer refuses for a converted read -- "roll", "rows" and the window "w", all
    three a periodic shift of a read at another location -- are left out of it: `operator.kinds` lists the steps kept,
    `operator.dropped` the kinds left out.
    With the two arguments unset the random stream and the program are what they were before the arguments existed."""
    rng = np.random.default_rng(seed)
    plan = []
    for _ in range(int(rng.integers(6, 14))):
        kind = rng.choice(["unary", "binary", "where", "minmax", "pow", "div", "roll", "rows", "param"])
        plan.append((kind, int(rng.integers(0, 1000)), int(rng.integers(0, 1000)), int(rng.integers(0, 1000)),
                     float(rng.uniform(-1.5, 1.5))))
    shifts = [tuple(int(a) for a in row) for row in rng.integers(-2, 3, size=(5, ndim))]
    frozen = [bool(v) for v in rng.integers(0, 4, size=5) == 0]
    axes = tuple(range(ndim))
    groups = [None] if out_locs is None else list(out_locs)
    locs = ("c" * ndim,) * 2 if locs is None else tuple(locs)
    converts = any(loc != (g or "c" * ndim) for loc in locs for g in groups)
    refused = ("roll", "rows") if converts else ()
    window = seed % 3 == 0 and not converts
    dropped = {str(kind) for kind, _, _, _, _ in plan if kind in refused} | ({"window"} if seed % 3 == 0 and converts else set())
    dropped = tuple(sorted(dropped))
    plan = [step for step in plan if step[0] not in refused]

    def group(ctx, loc, tag):
        m = ctx.mod
        idx, pts = ctx.indices(loc=loc), ctx.points(loc=loc)
        # (two dimensions: im is ix; four: the first axis of the tracer's layout has two or three points, too few to hold
        # a predicate worth folding, so the leading predicates sit on axis 1)
        it, im, ix = idx[1 if ndim == 4 else 0], idx[ndim // 2], idx[-1]
        vals = [ctx.field("a" if k % 2 == 0 else "b", *shifts[k], loc=loc, frozen=frozen[k] and k > 1) for k in range(5)]
        ramp = pts[0] * 0.7
        if ndim > 1:
            ramp = ramp + pts[1]
        if ndim > 2:
            ramp = ramp + pts[2] * 0.4
        if ndim > 3:
            ramp = ramp + pts[3] * 0.2
        vals += [ramp, ctx.cast(0.3)]
        coeff = ctx.field("coeff") if params else COEFF
        rows = ctx.extra
        for kind, i, j, k, c in plan:
            p, q, r = vals[i % len(vals)], vals[j % len(vals)], vals[k % len(vals)]
            if kind == "unary":
                f = [m.sin, m.cos, m.tanh, m.abs, m.square, lambda z: m.exp(m.clip(z, -3, 3)),
                     lambda z: m.sqrt(m.abs(z) + 0.5), lambda z: m.log(m.abs(z) + 0.5), m.relu, m.sigmoid][i % 10]
                vals.append(f(p * c))
            elif kind == "binary":
                vals.append([p + q, p - q * c, p * q, c - p, p * c + q][j % 5])
            elif kind == "where":
                cond = [it > 2, im == 0, p > q, (q < c) & (ix != 3), ~(p >= 0.1) | (it == 1)][k % 5]
                vals.append(m.where(cond, p, r * c))
            elif kind == "minmax":
                vals.append(m.maximum(p, q) - m.minimum(r, c))
            elif kind == "pow":
                vals.append([p**2, (m.abs(p) + 0.5) ** c, 1.5**(m.clip(q, -2, 2))][i % 3])
            elif kind == "roll":
                vals.append(m.roll(p + vals[0] * 0, (i % 5 - 2, j % 3 - 1, k % 3 - 1, (i + j) % 3 - 1)[:ndim], axis=axes) * c)
            elif kind == "rows":  # first / last rows imposed by concatenation (as heat_tmax / infer_constant do)
                full = p + vals[1] * 0
                vals.append(m.concatenate([rows[None], full[1:-1] * c, rows[None] * 0.5], axis=0))
            elif kind == "param":
                vals.append(p * coeff[k % 3] + coeff[(k + 1) % 3])
            else:
                vals.append(p / (2 + m.abs(q)) + c / (1.5 + q * q))
        outs = [("{}f{}".format(tag, n), v + vals[n] * 0.1) for n, v in enumerate(vals[-3:])]  # every output on the grid
        if window:
            lo, hi = (slice(1, None),), (slice(None, -1),)  # a window: one point less along the first and the last axis
            if ndim > 1:
                keep = (slice(None),) * (ndim - 2)
                lo, hi = lo + keep + (slice(None, -1),), hi + keep + (slice(1, None),)
            outs.append((tag + "w", outs[0][1][lo] - outs[1][1][hi]))
        return outs

    def operator(ctx):
        if len(groups) == 1:
            return group(ctx, groups[0], "")
        return [out for g, loc in enumerate(groups) for out in group(ctx, loc, "g{}".format(g))]

    operator.kinds = tuple(kind for kind, _, _, _, _ in plan)  # (the steps kept: a test may need a program without rolls)
    operator.dropped = dropped
    return operator


def random_case(seed, shape, dtype=np.float64, device="cpu"):
    """One random operator on plain fields, ready to run: (problem, state, operator, rows, arrays) -- two cell-centred
    `Field`s "a" and "b" on a grid of `shape` with a random state and random imposed rows, both drawn in `dtype` on the CPU
    (seeded by `seed`) and placed on `device`; `rows` and `arrays` (key -> array) are the same numbers widened to float64,
    for a reference."""
    import torch

    import odil_amd as odil

    ndim = len(shape)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    domain = odil.Domain(cshape=shape, dimnames=("t", "x", "y")[:ndim], dtype=dtype, multigrid=False)
    state = domain.init_state(odil.State(fields={"a": odil.Field(None, loc="c" * ndim), "b": odil.Field(None, loc="c" * ndim)}))
    gen = torch.Generator(device="cpu").manual_seed(100 + seed)
    rows = torch.randn(tuple(shape[1:]), generator=gen, dtype=torch.float64).to(tdt)
    arrays = [torch.randn(tuple(a.shape), generator=gen, dtype=torch.float64).to(tdt) for a in domain.arrays_from_state(state)]
    domain.arrays_to_state([a.to(device) for a in arrays], state)
    operator = random_operator(seed, params=False, ndim=ndim)
    problem = odil.Problem(operator, domain, extra=rows.to(device))
    return problem, state, operator, rows.double().numpy(), {k: a.double().numpy() for k, a in zip(("a", "b"), arrays)}
