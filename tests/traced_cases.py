"""Random straight-line programs (tests/random_ops.py) on grids large enough for the FOLDED copy of the generated kernels
to run (TEST INFRASTRUCTURE, no tests in here): the table of cases, the builder of one case, its float64 CPU reference
(oracle/odil_generic.py) and a census of the wavefronts that take the interior copy of every generated kernel
(stencil_codegen._interior_copy).  Shared by tests/test_traced_random_nd_host.py and tests/test_traced_random_nd_gpu.py
(the table CASES: everything on the cell grid, 1-D .. 3-D) and by tests/test_traced_staggered_host.py and
tests/test_traced_staggered_gpu.py (the table STAGGERED_CASES at the end: fields, reads and outputs at several locations,
2-D .. 4-D).

A wavefront of `k_fwd` or of a gather takes the folded copy only when none of its 64 x vw points has an exceptional index,
so the copy runs only on grids with rows or planes longer than a wavefront: the shapes below are the smallest of that kind
per dimension, per vector width (last extent a multiple of 4: four points per thread, else one) and per form of the index
prologue (last extent / vw a multiple of 64: wave-uniform leading indices)."""

import contextlib
import os
import re

import numpy as np
import torch

import odil_amd as odil
from odil_amd import stencil_jit
from odil_amd.stencil_codegen import _Codegen
from oracle import odil_generic as og
from oracle import odil_np as onp
from random_ops import random_operator

F32, F64 = np.float32, np.float64
_CHUNKED = (("ODIL_TRACE_CHUNK_MB", "0.05"),)  # (3, 64, 256): chunks of 16 rows of axis 1, XCD groups of 2 on 48 workgroups


class Case:
    def __init__(self, seed, shape, dtype=F64, multigrid=False, env=(), locs=None, out_locs=None, mg_nlvl=None):
        """locs: the locations of the fields "a" and "b", out_locs: the grids of the outputs (tests/random_ops.py; both None:
        everything on the cell grid), mg_nlvl: the levels of the multigrid fields (default 2)."""
        self.seed, self.shape, self.dtype, self.multigrid, self.env = seed, tuple(shape), dtype, bool(multigrid), tuple(env)
        self.locs, self.out_locs = None if locs is None else tuple(locs), None if out_locs is None else tuple(out_locs)
        self.mg_nlvl, self.levels = mg_nlvl, (mg_nlvl or 2) if multigrid else 1
        assert (locs is None) == (out_locs is None) and (mg_nlvl is None or multigrid)
        assert all(n % 2 ** (self.levels - 1) == 0 for n in shape), "every multigrid level halves the extents"

    @property
    def id(self):
        where = "" if self.locs is None else "-{}-{}".format(".".join(self.locs), "+".join(self.out_locs))
        return "s{}-{}-{}{}{}{}".format(self.seed, "x".join(map(str, self.shape)), "f32" if self.dtype == F32 else "f64",
                                        "-mg{}".format("" if self.levels == 2 else self.levels) if self.multigrid else "",
                                        "-chunked" if self.env else "", where)

    @property
    def field_locs(self):
        return self.locs or ("c" * self.ndim,) * 2

    @property
    def output_locs(self):
        return self.out_locs or ("c" * self.ndim,)

    @property
    def converts(self):
        """A read changes location: some field does not live on some output grid."""
        return any(a != b for a in self.field_locs for b in self.output_locs)

    @property
    def ndim(self):
        return len(self.shape)


# (seed, shape, dtype, multigrid, env): seeds >= 56 (0 .. 55 belong to tests/test_workloads_gpu.py), chosen so that the
# coverage conditions of tests/test_traced_random_nd_host.py hold -- a case that cannot meet them is replaced HERE
CASES = [
    Case(57, (1001,), F64),
    Case(61, (1001,), F32),
    Case(70, (1001,), F64),
    Case(83, (1001,), F64),
    Case(86, (1001,), F32),
    Case(94, (1001,), F64),
    Case(57, (40, 64), F64),
    Case(68, (40, 64), F32),
    Case(80, (40, 64), F64, True),
    Case(60, (40, 64), F64),
    Case(62, (40, 64), F32, True),
    Case(72, (40, 64), F64),
    Case(66, (20, 150), F64),
    Case(70, (20, 150), F32),
    Case(71, (20, 150), F64, True),
    Case(84, (20, 150), F64),
    Case(97, (20, 150), F32, True),
    Case(75, (20, 150), F64),
    Case(63, (12, 256), F64),
    Case(68, (12, 256), F32),
    Case(83, (12, 256), F64, True),
    Case(86, (12, 256), F64),
    Case(94, (12, 256), F32, True),
    Case(90, (12, 256), F64),
    Case(61, (10, 16, 64), F64),
    Case(76, (10, 16, 64), F32),
    Case(88, (10, 16, 64), F64, True),
    Case(69, (10, 16, 64), F64),
    Case(56, (10, 16, 64), F32, True),
    Case(78, (10, 16, 64), F64),
    Case(57, (10, 12, 150), F64),
    Case(71, (10, 12, 150), F32),
    Case(80, (10, 12, 150), F64, True),
    Case(87, (10, 12, 150), F64),
    Case(93, (10, 12, 150), F32, True),
    Case(99, (10, 12, 150), F64),
    Case(70, (6, 8, 256), F64),
    Case(84, (6, 8, 256), F32),
    Case(97, (6, 8, 256), F64, True),
    Case(81, (6, 8, 256), F64),
    Case(92, (6, 8, 256), F32, True),
    Case(98, (6, 8, 256), F64),
    Case(70, (3, 64, 256), F64, env=_CHUNKED),
    Case(73, (3, 64, 256), F32, env=_CHUNKED),
    Case(80, (3, 64, 256), F64, env=_CHUNKED),
    Case(84, (3, 64, 256), F64, env=_CHUNKED),
    Case(97, (3, 64, 256), F32, env=_CHUNKED),
    Case(99, (3, 64, 256), F64, env=_CHUNKED),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) <= 60


@contextlib.contextmanager
def environment(case, **more):
    """The environment variables of a case (and `more`) for the time of the block."""
    env = dict(case.env, **more)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(case, device=None, dtype=None):
    """(problem, state, operator, rows): the program `random_operator(seed, params=True, ndim, out_locs, locs)` on two fields
    "a", "b" at the case's locations (cell-centred by default; multigrid fields of the case's levels when it says so) and
    the `Array` "coeff", with random imposed rows of the shape of the first output grid without axis 0.  Every number is
    drawn on the CPU in float64 (seeded by the case's seed), rounded to the case's dtype and placed on `device` (default:
    the device of the current `mod`).  dtype=np.float64 on a float32 case: the float64 problem on the SAME float32-rounded
    numbers."""
    ndim, shape = case.ndim, case.shape
    dtype = dtype or case.dtype
    domain = odil.Domain(cshape=shape, dimnames=("t", "x", "y", "z")[:ndim], dtype=dtype, multigrid=case.multigrid,
                         mg_nlvl=case.levels if case.multigrid else None)
    assert not case.multigrid or domain.mg_nlvl == case.levels, "the extents do not allow the levels the case asks for"
    device = device or domain.mod.device
    state = odil.State(fields={"a": odil.Field(None, loc=case.field_locs[0]), "b": odil.Field(None, loc=case.field_locs[1]),
                               "coeff": odil.Array([0.7, -0.4, 1.3])})
    state = domain.init_state(state)
    rounded = torch.float64 if case.dtype == F64 else torch.float32
    final = torch.float64 if dtype == F64 else torch.float32
    gen = torch.Generator(device="cpu").manual_seed(100 + case.seed)
    draw = lambda s: torch.randn(tuple(s), generator=gen, dtype=torch.float64).to(rounded).to(final).to(device)
    rows = draw(domain.get_field_shape(case.output_locs[0])[1:])
    domain.arrays_to_state([draw(a.shape) for a in domain.arrays_from_state(state)], state)
    operator = random_operator(case.seed, params=True, ndim=ndim, out_locs=case.out_locs, locs=case.locs)
    return odil.Problem(operator, domain, extra=rows), state, operator, rows


_REFERENCE = dict()


def reference(case, problem, state, rows):
    """(loss, terms, grads in `arrays_from_state` order, output values, names) of the case in float64 on the CPU -- for a
    float32 case the float64 evaluation of the float32-rounded inputs.  Computed once per case, read-only."""
    if case.id not in _REFERENCE:
        _REFERENCE[case.id] = cpu_evaluation(case, problem, state, rows, np.float64)
    return _REFERENCE[case.id]


def cpu_evaluation(case, problem, state, rows, dtype):
    """(loss, terms, grads, values, names) of `oracle.odil_generic.eval_loss_grad` in `dtype` on the CPU, the results widened
    to float64 and read-only.  dtype=np.float32 on a float32 case (geometry, fields and rows in float): the evaluation
    whose distance from the float64 one says how much of the float32 bound rounding alone may use."""
    domain = problem.domain
    geom = og.Geometry(domain.cshape, domain.dimnames, np.asarray(domain.lower, dtype=dtype),
                       np.asarray(domain.upper, dtype=dtype), dtype)
    fields = og.fields_of_state(domain, state)
    for f in fields.values():
        for name in ("array", "terms"):
            if name in f:
                f[name] = [np.asarray(t, dtype=dtype) for t in f[name]] if name == "terms" else np.asarray(f[name], dtype=dtype)
    extra = rows.detach().cpu().to(torch.float64 if dtype == np.float64 else torch.float32)
    loss, grads, terms, names, values = og.eval_loss_grad(problem.operator, geom, fields, extra,
                                                          mg_axes=domain.mg_axes if case.multigrid else None)
    grads = [np.asarray(g, dtype=np.float64) for g in grads]
    values = [np.asarray(v, dtype=np.float64) for v in values]
    for a in grads + values:
        a.setflags(write=False)
    return (loss, tuple(terms), tuple(grads), tuple(values), tuple(names))


def measures(loss, terms, grads, ref):
    """(loss, terms, gradients, field gradients), plus the per-array figures: the loss and the worst term relative to the
    reference value; every gradient array in the max norm relative to the largest entry of ALL reference gradients; and the
    fields' arrays (all but the `Array` "coeff", the last) relative to the largest entry among themselves -- the gradient
    of a parameter is a sum over the grid, up to 1e4 times an entry of a field's gradient, and would hide an error of
    the gathers."""
    rloss, rterms, rgrads = ref[:3]
    to64 = lambda t: t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
    assert len(grads) == len(rgrads) and len(terms) == len(rterms)
    scale = max(float(np.max(np.abs(g))) for g in rgrads)
    fscale = max(float(np.max(np.abs(g))) for g in rgrads[:-1])
    assert np.isfinite(rloss) and rloss > 0 and fscale > 0 and all(r > 0 for r in rterms)
    errs = [float(np.max(np.abs(to64(g).reshape(r.shape) - r))) for g, r in zip(grads, rgrads)]
    e_loss = abs(float(loss) - rloss) / abs(rloss)
    e_term = max(abs(float(t) - r) / abs(r) for t, r in zip(terms, rterms))
    return (e_loss, e_term, max(errs) / scale, max(errs[:-1]) / fscale), ([e / scale for e in errs], [e / fscale for e in errs[:-1]])


def regular_arrays(problem, state):
    """key -> float64 array on the grid ("a", "b": the multigrid synthesis of their levels) or parameter vector ("coeff")."""
    fields = og.fields_of_state(problem.domain, state)
    out = dict()
    for key, f in fields.items():
        if f["kind"] == "mg":
            out[key] = onp.multigrid_to_regular([np.asarray(t, dtype=np.float64) for t in f["terms"]], f["loc"], f.get("factors"), None)
        else:
            out[key] = np.asarray(f["array"], dtype=np.float64)
    return out


# ---- census of the interior copies --------------------------------------------------------------------------------------
@contextlib.contextmanager
def interior_copies_recorded():
    """For the time of the block every `_Codegen._interior_copy` is recorded: a list of dicts kernel (name), nodes, vw,
    reverse, plan ((fold, exc, inbox) or None).  The generator itself is untouched afterwards."""
    calls, current = [], ["k_fwd"]
    copy, gather = _Codegen._interior_copy, _Codegen._gather_kernel

    def interior_copy(self, nodes, vw, reverse=False):
        res = copy(self, nodes, vw, reverse)
        calls.append(dict(kernel=current[0], nodes=list(nodes), vw=vw, reverse=reverse, plan=None if res is None else res[1]))
        return res

    def gather_kernel(self, S, name, *args, **kwargs):
        current[0] = name
        return gather(self, S, name, *args, **kwargs)

    _Codegen._interior_copy, _Codegen._gather_kernel = interior_copy, gather_kernel
    try:
        yield calls
    finally:
        _Codegen._interior_copy, _Codegen._gather_kernel = copy, gather


def thread_indices(cg, vw):
    """Grid indices of the first point of every thread in LAUNCH order (the wavefronts are consecutive groups of 64): the
    emitted lines of `_chunk_remap` evaluated as tests/test_stencil_jit_host.py::test_chunked_traversal_is_a_permutation does,
    then the decomposition of `_index_prologue`.  (The XCD remap of `_block_index` permutes whole workgroups.)"""
    shape = list(cg.GL)
    threads = int(np.prod(shape)) // vw
    S, env = [], dict(raw=np.arange(threads))
    cg._chunk_remap(S, shape, vw, "raw", "flat")
    for line in S:  # "const int a = e, b = e;": C's integer division of non-negative values is Python's //
        for name, expr in re.findall(r"(\w+) = ([^,;]+)", line.replace("const int ", "")):
            env[name] = eval(expr.replace("/", "//"), dict(), env)
    rem = env["flat"]
    assert sorted(rem.tolist()) == list(range(threads))
    idx = [None] * len(shape)
    for d in reversed(range(len(shape))):
        ext = shape[d] // vw if d == len(shape) - 1 else shape[d]
        idx[d] = (rem % ext if d else rem) * (vw if d == len(shape) - 1 else 1)
        rem = rem // ext
    assert idx[0].max() == shape[0] - 1
    return idx, not np.array_equal(env["flat"], env["raw"])


def wave_census(cg, vw, exc):
    """(wavefronts all of whose points avoid the exceptional indices `exc`, wavefronts in all) of a kernel with `vw` points
    per thread.  A wavefront is 64 x vw consecutive flat indices; lanes beyond the range do not vote."""
    idx, _ = thread_indices(cg, vw)
    last = len(idx) - 1
    ok = np.ones(idx[0].shape, dtype=bool)
    for d, values in exc.items():
        for p in range(vw if d == last else 1):
            ok &= ~np.isin(idx[d] + p, list(values))
    waves = -(-ok.size // 64)
    ok = np.concatenate([ok, np.ones(waves * 64 - ok.size, dtype=bool)]).reshape(waves, 64)
    return int(ok.all(axis=1).sum()), waves


def census(problem, state, only=None):
    """(cg, source, kernels): the generator after `source()` and, per generated kernel that may have an interior copy, a dict
    kernel, nodes, vw, reverse, plan, interior (wavefronts that take the folded copy), waves (all), remapped (chunk remap
    in force), uniform (wave-uniform index prologue emitted).  only: the positions of one shape group of the outputs."""
    tr, outs, raw, names, G = stencil_jit.trace_outputs(problem, state, only)
    cg = _Codegen(tr, outs, raw, G, state)
    with interior_copies_recorded() as calls:
        source = cg.source()
    starts = {c["kernel"]: source.index("void {}(const Args a".format(c["kernel"])) for c in calls}
    for c in calls:
        _, c["remapped"] = thread_indices(cg, c["vw"])
        end = source.find('extern "C"', starts[c["kernel"]])
        text = source[starts[c["kernel"]]:end if end >= 0 else len(source)]
        c["uniform"] = "__builtin_amdgcn_readfirstlane(" in text.split("__all(")[0]
        c["interior"], c["waves"] = (0, None) if c["plan"] is None else wave_census(cg, c["vw"], c["plan"][1])
        if c["plan"] is None:
            c["waves"] = -(-(int(np.prod(cg.GL)) // c["vw"]) // 64)
        assert ("__all((int)(" in text) == (c["plan"] is not None), c["kernel"]
    return cg, source, calls


def census_groups(problem, state):
    """[(cg, source, kernels)], one per kernel set: an operator whose outputs live on grids of several shapes is traced
    once per shape group, as `stencil_jit.TracedGroups` does."""
    try:
        return [census(problem, state)]
    except stencil_jit.TraceGroups as e:
        return [census(problem, state, only=positions) for positions in e.groups]


def both_copies(kernel):
    return kernel["plan"] is not None and 0 < kernel["interior"] < kernel["waves"]


# the cases that also run with every output differentiated in registers (ODIL_TRACE_RECOMPUTE=0) and with every output
# that can be re-evaluated by the gathers (ODIL_TRACE_RECOMPUTE_ALL=1): four per dimension, each with a gather that runs
# both of its copies in the default mode
RECOMPUTE_CASES = [
    "s61-1001-f32", "s70-1001-f64", "s83-1001-f64", "s94-1001-f64",
    "s57-40x64-f64", "s80-40x64-f64-mg", "s71-20x150-f64-mg", "s68-12x256-f32",
    "s88-10x16x64-f64-mg", "s57-10x12x150-f64", "s97-6x8x256-f64-mg", "s80-3x64x256-f64-chunked",
]
RECOMPUTE_MODES = {"all_legacy": dict(ODIL_TRACE_RECOMPUTE="0"), "all_recomputed": dict(ODIL_TRACE_RECOMPUTE_ALL="1")}
assert all(i in BY_ID for i in RECOMPUTE_CASES)


def adam_prediction(case, cg):
    """(done, why): how many leading arrays of the state `TracedOperator.eval_loss_grad_adam` updates inside the gathers, from
    the layout of the state ("a", "b": one array each, or two multigrid levels; then "coeff") and what was generated.  A
    field is updated in its gather when it has one (a field whose only adjoint array already IS its gradient has none) and,
    for a plain `Field`, when no gather of the epoch re-reads the array the update would overwrite; the fields after the
    first that is not are left to the optimizer.  done == 0: the call returns None."""
    reread = {k for keys in cg.gather_reads_sources.values() for k in keys}
    done, per = 0, case.levels
    for key in ("a", "b"):
        if key not in cg.gathers:
            return done, "'{}' has no gather (its stored adjoint is its gradient)".format(key)
        if not case.multigrid and key in reread:
            return done, "a gather re-reads the plain field '{}'".format(key)
        done += per
    return done, "both fields are updated by their gathers; 'coeff' is left to the optimizer"


# Adam inside the gathers (ODIL_FUSE_ADAM_SMALL=1), two cases per dimension: plain fields and multigrid fields, one and
# four points per thread, and one whose gathers re-read the field they would update (nothing fuses: the call returns None)
ADAM_CASES = ["s61-1001-f32", "s70-1001-f64", "s80-40x64-f64-mg", "s97-20x150-f32-mg", "s76-10x16x64-f32", "s80-10x12x150-f64-mg"]
assert all(i in BY_ID for i in ADAM_CASES)


# ---- the staggered and four-dimensional table ------------------------------------------------------------------------------
# Fields that do not live on the grid of the outputs (every read pads 'c' -> 'n' or trims 'n' -> 'c', the gathers are the
# irregular ones), node-centred grids with odd extents, outputs on two grids (one kernel set each) and the (t, x, y, z)
# layout of the tracer problem: four `nccc` arrays ARE its unknowns.  Seeds >= 100 (0 .. 99 belong to the tables above);
# the shapes are the smallest per row for which the conditions of tests/test_traced_staggered_host.py hold (a wavefront of
# `k_fwd` with no exceptional index beside one with), at most 50 000 points each; a case that cannot meet them is replaced HERE
_MG3 = dict(multigrid=True, mg_nlvl=3)
_CHUNKED_4D = (("ODIL_TRACE_CHUNK_MB", "0.05"),)  # (3, 16, 16, 64): chunks of axis 1
STAGGERED_CASES = [
    # G = 41 x 65, one point per thread, both fields padded along one axis each
    Case(100, (40, 64), F64, locs=("nc", "cn"), out_locs=("nn",)),
    Case(105, (40, 64), F64, locs=("nc", "cn"), out_locs=("nn",)),
    Case(110, (40, 64), F32, locs=("nc", "cn"), out_locs=("nn",)),
    # three multigrid levels with a node axis (13, 7, 4 rows), four points per thread, wave-uniform prologue
    Case(105, (12, 256), F64, locs=("cc", "nc"), out_locs=("nc",), **_MG3),
    Case(110, (12, 256), F32, locs=("cc", "nc"), out_locs=("nc",), **_MG3),
    Case(116, (12, 256), F64, locs=("cc", "nc"), out_locs=("nc",), **_MG3),
    # two kernel sets: each field is regular in one of them, padded or trimmed in the other
    Case(105, (16, 64), F64, locs=("cc", "nc"), out_locs=("cc", "nc")),
    Case(113, (16, 64), F32, locs=("cc", "nc"), out_locs=("cc", "nc")),
    Case(105, (10, 16, 64), F64, locs=("ccc", "ncc"), out_locs=("ccc", "ncc")),
    # three dimensions: trimmed reads along the first and the last axis
    Case(100, (10, 16, 64), F64, locs=("ncc", "ccn"), out_locs=("ccc",)),
    Case(105, (10, 16, 64), F32, locs=("ncc", "ccn"), out_locs=("ccc",)),
    # ... padded and trimmed reads in one program, one point per thread
    Case(100, (10, 12, 150), F64, locs=("ccc", "ncn"), out_locs=("ncc",)),
    Case(105, (10, 12, 150), F32, locs=("ccc", "ncn"), out_locs=("ncc",)),
    Case(109, (10, 12, 150), F64, locs=("ccc", "ncn"), out_locs=("ncc",)),
    # the tracer's layout, G = 3 x 8 x 8 x 64: nothing converts, so rolls, imposed rows and windows stay in the programs
    Case(150, (2, 8, 8, 64), F32, locs=("nccc", "nccc"), out_locs=("nccc",)),
    Case(105, (2, 8, 8, 64), F64, locs=("nccc", "nccc"), out_locs=("nccc",)),
    Case(123, (2, 8, 8, 64), F64, locs=("nccc", "nccc"), out_locs=("nccc",)),
    # four dimensions, a trimmed first axis: wave-uniform prologue / a last extent that is no multiple of 64
    Case(100, (2, 4, 8, 256), F64, locs=("nccc", "cccc"), out_locs=("cccc",)),
    Case(105, (2, 4, 8, 256), F32, locs=("nccc", "cccc"), out_locs=("cccc",)),
    Case(100, (2, 4, 8, 152), F64, locs=("nccc", "ccnc"), out_locs=("cccc",)),
    Case(110, (2, 4, 8, 152), F32, locs=("nccc", "ccnc"), out_locs=("cccc",)),
    # multigrid `nccc` fields (two levels: 5 and 3 time levels): the transposes come after the merged gather
    Case(102, (4, 8, 8, 64), F64, True, locs=("nccc", "nccc"), out_locs=("nccc",)),
    Case(105, (4, 8, 8, 64), F32, True, locs=("nccc", "nccc"), out_locs=("nccc",)),
    Case(123, (4, 8, 8, 64), F64, True, locs=("nccc", "nccc"), out_locs=("nccc",)),
    # the chunk remap with a fourth index
    Case(100, (2, 16, 16, 64), F64, env=_CHUNKED_4D, locs=("nccc", "nccc"), out_locs=("nccc",)),
    Case(105, (2, 16, 16, 64), F32, env=_CHUNKED_4D, locs=("nccc", "nccc"), out_locs=("nccc",)),
    # cell-centred fields, node-centred outputs: EVERY read converts
    Case(105, (40, 64), F64, locs=("cc", "cc"), out_locs=("nn",)),
    Case(113, (40, 64), F32, locs=("cc", "cc"), out_locs=("nn",)),
]
STAGGERED_BY_ID = {c.id: c for c in STAGGERED_CASES}
assert len(STAGGERED_BY_ID) == len(STAGGERED_CASES) <= 28 and not set(STAGGERED_BY_ID) & set(BY_ID)
assert all(c.seed >= 100 and int(np.prod(c.shape)) <= 50000 for c in STAGGERED_CASES)


def conversions(cg, state):
    """(a live read pads 'c' -> 'n', a live read trims 'n' -> 'c', the fields whose gather is the irregular one) of one
    kernel set: what the staggered table is there to reach."""
    pairs = [(f, l) for n in cg.tr.nodes if n.op == "read" and n.attr[0] in state.fields
             for f, l in zip(state.fields[n.attr[0]].loc, n.attr[2])]
    irregular = sorted(key for key in cg.gathers if tuple(cg._field_shape(key)) != tuple(cg.G))
    return ("c", "n") in pairs, ("n", "c") in pairs, irregular


# two cases per dimension that also run in the two other recompute modes
STAGGERED_RECOMPUTE_CASES = [
    "s105-40x64-f64-nc.cn-nn", "s105-16x64-f64-cc.nc-cc+nc",
    "s100-10x16x64-f64-ncc.ccn-ccc", "s109-10x12x150-f64-ccc.ncn-ncc",
    "s123-2x8x8x64-f64-nccc.nccc-nccc", "s100-2x4x8x152-f64-nccc.ccnc-cccc",
]
# Adam inside the gathers on the tracer's layout (every field regular): plain fields that no gather re-reads, and multigrid
# fields whose merged gather runs both of its copies
STAGGERED_ADAM_CASES = ["s150-2x8x8x64-f32-nccc.nccc-nccc", "s123-4x8x8x64-f64-mg-nccc.nccc-nccc"]
assert all(i in STAGGERED_BY_ID for i in STAGGERED_RECOMPUTE_CASES + STAGGERED_ADAM_CASES)
