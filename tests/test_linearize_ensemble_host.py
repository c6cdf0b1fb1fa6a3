"""Host checks of the batched linearisation of Newton ensembles (`odil_amd.ensemble.linearize_ensemble`), no GPU:

1  generator: `_Codegen(..., jac="batch")` adds `k_jac_batch` and its launcher behind a source that holds the `jac=True`
   source's `k_jac` unchanged; the two kernels share their body line for line; `jac=True` emits what it emitted; a slab
   rank refuses the batched form
2  the batched source builds for gfx950 (where hipcc is present: a compile, nothing more)
3  `gmg.stencil_slot_plan` on hand-written item lists, against `gmg.stencil_coefficients` on the same items
4  `linearize_ensemble` refuses members by name before anything is traced

The operator is that of examples/diffusion/ensemble.py, traced on CPU tensors as tests/test_jacobian_kernel_host.py does."""

import importlib.util
import os
import shutil
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT

import odil_amd as odil
from odil_amd import gmg, jit_cache, runtime, stencil_jit
from odil_amd.stencil_codegen import _Codegen
from odil_amd.stencil_trace import TraceUnsupported

SPECS = ["--ndim {} --N 16{}".format(nd, beta) for nd in (1, 2, 3) for beta in ("", " --beta 1")]


def diffusion_ensemble():
    """examples/diffusion/ensemble.py under a name of its own: examples/poisson has an `ensemble` module too, and whichever
    is imported first under that name stays in `sys.modules` for every test that follows."""
    name = "diffusion_ensemble_example"
    if name not in sys.modules:
        path = os.path.join(ROOT, "examples", "diffusion")
        if path not in sys.path:
            sys.path.append(path)  # (for its `import diffusion`)
        spec = importlib.util.spec_from_file_location(name, os.path.join(path, "ensemble.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


@pytest.fixture()
def cpu_mod():
    saved, saved_log = runtime._mod, odil.util.g_log_file
    runtime._mod = odil.ModRocm(device="cpu")
    odil.util.set_log_file(open(os.devnull, "w"))
    yield runtime._mod
    runtime._mod = saved
    odil.util.g_log_file = saved_log


def member(spec, b=0, nb=4):
    ensemble = diffusion_ensemble()
    args = ensemble.parse_args((spec + " --members {}".format(nb)).split())
    return ensemble.make_member(args, b)


def generate(problem, state, jac, slab=None):
    tr, outs, raw, names, G = stencil_jit.trace_outputs(problem, state)
    cg = _Codegen(tr, outs, raw, G, state, slab=slab, jac=jac)
    return cg, cg.source()


def kernel_lines(source, name):
    """The lines of `extern "C" __global__ ... void name(` up to its closing brace."""
    lines = source.split("\n")
    first = next(i for i, line in enumerate(lines) if line.startswith('extern "C" __global__') and " {}(".format(name) in line)
    last = next(i for i in range(first, len(lines)) if lines[i] == "}")
    return lines[first:last + 1]


# ------------------------------------------------------------------------------------------------------- 1: generator
@pytest.mark.parametrize("spec", SPECS)
def test_batch_source_holds_the_single_kernel_and_shares_its_body(cpu_mod, spec):
    problem, state = member(spec)
    cg1, single = generate(problem, state, True)
    cg2, batch = generate(problem, state, "batch")
    assert "k_jac_batch" not in single and "jit_jac_batch" not in single
    assert cg1.jac_items == cg2.jac_items and cg1.jac_blocks == cg2.jac_blocks
    one = kernel_lines(single, "k_jac")
    assert kernel_lines(batch, "k_jac") == one, "k_jac of the batched source differs"
    many = kernel_lines(batch, "k_jac_batch")
    assert "const Args* __restrict__ ab, const JacP* __restrict__ jb" in many[0]
    prologue = next(i for i, line in enumerate(many) if line.startswith("  const AdamP ad"))
    assert prologue <= 3 and all("blockIdx.y" in line for line in many[1:prologue])
    assert many[prologue + 1:] == one[1:], "the bodies differ"
    assert not any("blockIdx.y" in line for line in one)
    # everything ahead of the batched kernel is the single source's text, and only the launcher follows its own
    cut = single.index('extern "C" int jit_fwd(')
    assert batch.startswith(single[:cut])
    assert 'extern "C" int jit_jac_batch(const void* args_dev, const void* ptrs_dev, int nmembers, void* stream)' in batch
    assert "dim3({}, nmembers)".format(cg2.jac_blocks) in batch


@pytest.mark.parametrize("spec", SPECS[:2] + SPECS[4:])
def test_sources_without_the_batched_kernel_do_not_change(cpu_mod, spec):
    """jac=True / jac=False emit the same bytes whether or not a batched source was generated from the same trace before
    (the library hash is the hash of the text: tools/prebuild_jit.py)."""
    problem, state = member(spec)
    before = [generate(problem, state, jac)[1] for jac in (False, True)]
    generate(problem, state, "batch")
    assert [generate(problem, state, jac)[1] for jac in (False, True)] == before
    assert "k_jac" not in before[0]


def test_slab_rank_refuses_the_batched_kernel(cpu_mod):
    problem, state = member("--ndim 3 --N 16")
    with pytest.raises(TraceUnsupported, match="batched Jacobian kernel of a slab rank"):
        generate(problem, state, "batch", slab=(0, 8))
    generate(problem, state, True, slab=(0, 8))  # (the single form of a slab rank stays)


# --------------------------------------------------------------------------------------------------------- 2: compile
@pytest.mark.parametrize("spec", ["--ndim 2 --N 16 --beta 1", "--ndim 3 --N 16 --double 0"])
def test_batch_source_compiles_for_gfx950(cpu_mod, spec):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc here: the batched source is not compiled")
    problem, state = member(spec)
    cg, source = generate(problem, state, "batch")
    lib, path = jit_cache._compile(source, cg.flags)
    assert os.path.exists(path) and hasattr(lib, "jit_jac_batch") and hasattr(lib, "jit_jac")


# ------------------------------------------------------------------------------------------------------- 3: slot plan
def items_of(shifts, key="u", out=0):
    nd = len(shifts[0]) if shifts else 0
    return [(out, None)] + [(out, (key, tuple(s), "c" * nd, False)) for s in shifts]


def test_slot_plan_of_a_permuted_read_order():
    shifts = [(0, 1), (0, 0), (-1, 0), (0, -1), (1, 0)]
    plan = gmg.stencil_slot_plan(items_of(shifts), (8, 12))
    assert plan.slots == [None, 4, 0, 1, 3, 2] and plan.missing == [] and plan.single is None
    # shifts are taken modulo the extents, as the periodic roll takes them
    plan = gmg.stencil_slot_plan(items_of([(0, 0), (7, 0), (-7, 0), (0, 11), (0, -11)]), (8, 12))
    assert plan.slots == [None, 0, 1, 2, 3, 4]
    # the value may stand anywhere among the items
    mixed = items_of(shifts)
    mixed = mixed[1:3] + mixed[:1] + mixed[3:]
    assert gmg.stencil_slot_plan(mixed, (8, 12)).slots == [4, 0, None, 1, 3, 2]


def test_slot_plan_missing_shift_is_a_zero_slot():
    plan = gmg.stencil_slot_plan(items_of([(0, 0, 0), (0, -1, 0), (0, 0, 1)]), (4, 6, 8))
    assert plan.slots == [None, 0, 3, 6] and plan.missing == [1, 2, 4, 5] and plan.single is None


def test_slot_plan_duplicate_shift_keeps_the_member_single():
    # +3 and -1 on an extent of 4 are the same neighbour: `stencil_coefficients` sums the two arrays
    plan = gmg.stencil_slot_plan(items_of([(0, 0), (-1, 0), (3, 0), (1, 0)]), (4, 6))
    assert plan.single is not None and "summed" in plan.single and "(-1, 0)" in plan.single
    assert plan.slots == [None, 0, 1, 1, 2]


@pytest.mark.parametrize("items,shape,reason", [
    (items_of([(0, 0), (2, 0)]), (4, 6), "not a point of the"),                  # +2 on an extent of 4: no unit vector
    (items_of([(0, 0), (1, 1)]), (8, 8), "not a point of the"),                  # a diagonal
    (items_of([(0, 0)]) + items_of([(0, 0)], out=1), (8, 8), "2 outputs"),
    (items_of([(1, 0), (-1, 0)]), (8, 8), "the cell itself"),                    # (the centre is missing)
    (items_of([(0, 0)]), (3, 8), "extents of at least 4"),
    (items_of([(0, 0, 0, 0)]), (4, 4, 4, 4), "at most three dimensions"),
    ([(0, None), (0, ("u", (0, 0), "nc", False))], (8, 8), "not a point of the"),
], ids=["shift2-extent4", "diagonal", "two-outputs", "no-centre", "extent3", "4-D", "node-centred-read"])
def test_slot_plan_refuses_what_recognise_stencil_refuses(items, shape, reason):
    with pytest.raises(ValueError, match=reason):
        gmg.stencil_slot_plan(items, shape)
    # ... and `stencil_coefficients` answers the same shifts with None
    shifts = [(attr[1], torch.zeros(shape)) for k, attr in items if attr is not None and k == 0]
    if reason in ("not a point of the", "the cell itself") and items[-1][1][2] == "c" * len(shape):
        assert gmg.stencil_coefficients(shifts, shape) is None


def test_slot_plan_refuses_other_fields():
    with pytest.raises(ValueError, match="not one cell-centred field"):
        gmg.stencil_slot_plan(items_of([(0, 0)]), (8, 8), fields=dict(u="cc", v="cc"))
    with pytest.raises(ValueError, match="not one cell-centred field"):
        gmg.stencil_slot_plan(items_of([(0, 0)]), (8, 8), fields=dict(u="nc"))
    assert gmg.stencil_slot_plan(items_of([(0, 0)]), (8, 8), fields=dict(u="cc")).missing == [1, 2, 3, 4]


@pytest.mark.parametrize("shifts,shape", [
    ([(0, 1), (0, 0), (-1, 0), (0, -1), (1, 0)], (5, 7)),
    ([(0,), (63,), (1,)], (64,)),
    ([(0, 0, 0), (0, -1, 0), (0, 0, 1), (3, 0, 0)], (4, 6, 8)),
], ids=["2d-permuted", "1d-wrapped", "3d-missing"])
def test_slot_plan_agrees_with_stencil_coefficients(shifts, shape):
    """Arrays stored where the plan says are the tensor `stencil_coefficients` builds from the same items."""
    rng = np.random.default_rng(3)
    arrays = [torch.tensor(rng.standard_normal(shape)) for _ in shifts]
    want = gmg.stencil_coefficients(list(zip(shifts, arrays)), shape)
    plan = gmg.stencil_slot_plan(items_of(shifts), shape)
    assert plan.single is None
    got = torch.full((2 * len(shape) + 1,) + tuple(shape), float("nan"), dtype=torch.float64)
    for slot in plan.missing:
        got[slot].zero_()
    for slot, a in zip(plan.slots[1:], arrays):
        got[slot].copy_(a)
    assert torch.equal(got, want)


# -------------------------------------------------------------------------------------------------------- 4: refusals
def test_linearize_ensemble_refuses_members_by_name_before_tracing(cpu_mod, monkeypatch):
    def no_trace(*args, **kwargs):
        raise AssertionError("an operator was traced before the members were checked")

    monkeypatch.setattr(stencil_jit, "trace_jacobian", no_trace)
    monkeypatch.setattr(stencil_jit, "trace_outputs", no_trace)
    spec = "--ndim 2 --N 16"
    built = [member(spec, b, 3) for b in range(3)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    with pytest.raises(ValueError, match="linearize_ensemble: 3 problems with 2 states"):
        odil.util.linearize_ensemble(problems, states[:2])
    swapped = list(built)
    swapped[1] = member(spec + " --multigrid 1", 1, 3)
    with pytest.raises(ValueError, match="linearize_ensemble: member 1: the unknown is a MultigridField"):
        odil.util.linearize_ensemble([p for p, _ in swapped], [s for _, s in swapped])
    swapped[1], swapped[2] = built[1], member("--ndim 2 --N 8", 2, 3)
    with pytest.raises(ValueError, match="linearize_ensemble: member 2: cells .* differ from member 0's"):
        odil.util.linearize_ensemble([p for p, _ in swapped], [s for _, s in swapped])
    swapped[2] = member(spec + " --double 0", 2, 3)
    with pytest.raises(ValueError, match="linearize_ensemble: member 2: dtype .* differ from member 0's"):
        odil.util.linearize_ensemble([p for p, _ in swapped], [s for _, s in swapped])
    with pytest.raises(ValueError, match="linearize_ensemble: member 0: .*4 cells per axis"):
        odil.util.linearize_ensemble(*[[x] for x in member("--ndim 2 --N 2", 0, 1)])


def test_driver_refuses_an_unknown_linearize(cpu_mod):
    ensemble = diffusion_ensemble()
    args = ensemble.parse_args("--ndim 2 --N 16 --members 1".split())
    problem, state = ensemble.make_member(args, 0)
    with pytest.raises(ValueError, match="linearize 'gpu'"):
        odil.util.optimize_newton_ensemble(args, [problem], [state], linearize="gpu")
