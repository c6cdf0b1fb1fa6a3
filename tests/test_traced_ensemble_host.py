"""Host checks of the Adam ensembles of traced stencil operators (`odil.util.optimize_ensemble` beyond the Poisson stencil,
`fused.TracedLaunchEnsemble`, `stencil_bind.EpochBatch`), no GPU:

1  generator: `_Codegen(..., batch=True)` adds `k_fwd_batch`, `k_final_batch`, `k_loss_batch`, the batched gathers and their
   launchers to a source that is otherwise the text of the single source; every batched kernel shares its body line for
   line with its single kernel; without the switch the source is what it was
2  the generator refuses a marching forward kernel, a slab rank, network / Array parameters and outputs in parameter space
3  the driver's structural refusals name the right member before anything is traced, and leave the states alone
4  the batched source of the diffusion operator builds for gfx950 (where hipcc is present: a compile, nothing more)

Operators are traced on CPU tensors, as tests/test_linearize_ensemble_host.py does."""

import os
import shutil
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT
from traced_ensemble_members import make_member, make_members, run_args, two_outputs

import odil_amd as odil
from odil_amd import fused, jit_cache, runtime, stencil_bind, stencil_jit
from odil_amd.stencil_codegen import _Codegen
from odil_amd.stencil_trace import TraceUnsupported

for sub in ("heat", "velocity_from_tracer"):
    sys.path.insert(0, os.path.join(ROOT, "examples", sub))

CASES = [((64,), 3, 0.0), ((16, 16), 3, 1.0), ((12, 18), 2, 0.0), ((8, 512), 2, 1.0), ((8, 8, 8), 2, 0.0), ((16, 16), None, 1.0)]


@pytest.fixture()
def cpu_mod():
    saved, saved_log = runtime._mod, odil.util.g_log_file
    runtime._mod = odil.ModRocm(device="cpu")
    odil.util.set_log_file(open(os.devnull, "w"))
    yield runtime._mod
    runtime._mod = saved
    odil.util.g_log_file = saved_log


def generate(problem, state, batch, slab=None, jac=False):
    tr, outs, raw, names, G = stencil_jit.trace_outputs(problem, state)
    cg = _Codegen(tr, outs, raw, G, state, slab=slab, jac=jac, batch=batch)
    return cg, cg.source()


def kernel_lines(source, name):
    """The lines of `extern "C" __global__ ... void name(` up to its closing brace."""
    lines = source.split("\n")
    first = next(i for i, line in enumerate(lines) if line.startswith('extern "C" __global__') and " {}(".format(name) in line)
    last = next(i for i in range(first, len(lines)) if lines[i] == "}")
    return lines[first:last + 1]


def body_after_head(many, member):
    """The lines of a batched kernel behind its head: the signature, the member's argument block (and, in a gather, its
    GatB, AdamP and pointers), each of which names the member's grid dimension or the struct read through it."""
    k = 1
    while many[k].startswith(("  Args a;", "  __builtin_memcpy(&a, (ArgsC*)(ab + ", "  GatB gp;", "  __builtin_memcpy(&gp, (GatBC*)(gb + ",
                              "  const AdamP ad = gp.ad;", "  T* __restrict__ g = gp.", "  GatAll ga;", "  ga.g[")):
        k += 1
    assert "ab + " + member in many[2]
    return many[k:]


# ------------------------------------------------------------------------------------------------------- 1: generator
@pytest.mark.parametrize("cshape,nlvl,beta", CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batched_kernels_share_the_bodies_of_the_single_kernels(cpu_mod, cshape, nlvl, beta, dtype):
    problem, state = make_member(cshape, nlvl, dtype, 0, 3, beta=beta)
    cg1, single = generate(problem, state, False)
    cg2, batch = generate(problem, state, True)
    assert "_batch" not in single
    assert cg1.gathers == cg2.gathers and cg1.direct == cg2.direct and cg1.fwd_blocks == cg2.fwd_blocks
    assert cg2.gathers, "the diffusion operator reads shifted values: its field has a gather"
    for name, member in [("k_fwd", "blockIdx.y"), ("k_final", "blockIdx.z"), ("k_loss", "blockIdx.x")] + [
            ("k_gat_{}".format(gi), "blockIdx.y") for gi in range(len(cg2.gathers))]:
        one = kernel_lines(single, name)
        assert kernel_lines(batch, name) == one, "{} of the batched source differs".format(name)
        many = kernel_lines(batch, name + "_batch")
        assert many[0].startswith('extern "C" __global__ ' + one[0].split()[3] + " void " + name + "_batch(const Args* __restrict__ ab")
        assert body_after_head(many, member) == one[1:], "the bodies of {} differ".format(name)
        assert not any(member in line for line in one), "{} reads the grid dimension that counts the members".format(name)
    # the text around the batched kernels is the single source's: they stand between the gathers and the launchers,
    # their own launchers at the end
    cut = single.index('extern "C" int jit_fwd(')
    assert batch.startswith(single[:cut])
    rest = batch[cut:]
    at = rest.index(single[cut:])
    assert "k_fwd_batch" in rest[:at] and "jit_" not in rest[:at]
    tail = rest[at + len(single[cut:]):]
    assert tail.startswith('extern "C" int jit_fwd_batch(const void* args_dev, int nmembers, void* stream) {')
    assert 'extern "C" int jit_gather_batch(int which, const void* args_dev, const void* ptrs_dev, int nmembers, void* stream) {' in tail
    assert tail.count("if (nmembers < 1 || nmembers > 65535) return -1;") == 2
    assert "k_fwd_batch, dim3({}, nmembers), dim3(256)".format(cg2.fwd_blocks) in tail
    assert "k_final_batch, dim3(1, SEG, nmembers)" in tail and "k_loss_batch, dim3(nmembers), dim3(64)" in tail
    for gi in range(len(cg2.gathers)):
        assert "k_gat_{0}_batch, dim3({1}, nmembers)".format(gi, cg2.gather_blocks[gi]) in tail
    # the members' blocks are read through the constant address space, as k_jac_batch reads them
    assert "typedef const __attribute__((address_space(4))) Args ArgsC;" in batch
    assert set(stencil_bind._ARGTYPES) >= {"jit_fwd_batch", "jit_gather_batch"}


def test_sources_without_the_switch_do_not_change(cpu_mod):
    """batch=False emits the same bytes whether or not a batched source was generated from the same trace before, with and
    without the Jacobian kernels (the library hash is the hash of the text)."""
    problem, state = make_member((16, 16), None, np.float64, 0, 2, beta=1.0)
    before = [generate(problem, state, False, jac=jac)[1] for jac in (False, True, "batch")]
    generate(problem, state, True)
    assert [generate(problem, state, False, jac=jac)[1] for jac in (False, True, "batch")] == before
    both = generate(problem, state, True, jac="batch")[1]  # (the two batched forms in one source: one ArgsC, twice the same)
    assert "k_jac_batch" in both and "k_fwd_batch" in both


def test_two_outputs_reach_the_batched_reductions(cpu_mod):
    problem, state = make_member((16, 16), 3, np.float64, 0, 2, operator=two_outputs)
    cg, batch = generate(problem, state, True)
    assert len(cg.outputs) == 2 and "k_final_batch, dim3(2, SEG, nmembers)" in batch
    assert body_after_head(kernel_lines(batch, "k_loss_batch"), "blockIdx.x") == kernel_lines(batch, "k_loss")[1:]


def test_merged_gather_has_a_batched_form(cpu_mod):
    """Two fields with symbolic gathers: `k_gat_all_batch` runs the body of `k_gat_all` on a GatAll built from the member's
    GatB.  (The driver admits one unknown; the generator serves the form all the same.)"""
    import veltracer

    problem, state = veltracer.make_problem(veltracer.parse_args(["--Nt", "8", "--Nx", "16", "--Ny", "16"]))
    cg, batch = generate(problem, state, True)
    assert len(cg.merged) >= 2
    many, one = kernel_lines(batch, "k_gat_all_batch"), kernel_lines(batch, "k_gat_all")
    assert body_after_head(many, "blockIdx.y") == one[1:]
    assert "case -1: hipLaunchKernelGGL(k_gat_all_batch, dim3({}, nmembers)".format(cg.gather_all_blocks) in batch


# ------------------------------------------------------------------------------------------- 2: the generator's refusals
def test_generator_refuses_what_is_no_pointwise_body(cpu_mod, monkeypatch):
    problem, state = make_member((8, 8, 8), 2, np.float64, 0, 2)
    with pytest.raises(TraceUnsupported, match="batched forward and gather kernels of a slab rank"):
        generate(problem, state, True, slab=(0, 4))
    generate(problem, state, False, slab=(0, 4))  # (the single form of a slab rank stays)
    import heat2d

    hargs = ["--Nt", "8", "--Nx", "16", "--Ny", "128", "--infer_k", "1", "--imposed", "stripe", "--multigrid", "0"]
    monkeypatch.setenv("ODIL_TRACE_SHARE", "0")  # a pointwise network: parameter gradients reduced over the grid
    with pytest.raises(TraceUnsupported, match="network or Array parameters"):
        generate(*heat2d.make_problem(heat2d.parse_args(hargs)), True)
    with pytest.raises(TraceUnsupported, match="network or Array parameters"):
        stencil_jit.TracedOperator(*heat2d.make_problem(heat2d.parse_args(hargs)), batch=True)
    monkeypatch.setenv("ODIL_TRACE_SHARE", "march")
    with pytest.raises(TraceUnsupported, match="marching forward kernel"):
        generate(*heat2d.make_problem(heat2d.parse_args(hargs)), True)
    # an output in parameter space
    domain = odil.Domain(cshape=(8, 8), dtype=np.float64)
    pstate = odil.State()
    pstate.fields["u"] = odil.Field(None, loc="cc")
    pstate.fields["p"] = odil.Array(np.array([1.0, -2.0, 0.5]))
    pstate = domain.init_state(pstate)
    op = lambda ctx: [ctx.field("u") - ctx.field("u", 1, 0), ctx.domain.arrays_from_field(ctx.state.fields["p"])[0] * 2.0]
    stencil_jit.TracedOperator(odil.Problem(op, domain), pstate)
    with pytest.raises(TraceUnsupported, match="outputs in parameter space"):
        stencil_jit.TracedOperator(odil.Problem(op, domain), pstate, batch=True)


# ---------------------------------------------------------------------------------------------- 3: the driver's refusals
def _arrays(state):
    return [getattr(box, at) if isinstance(at, str) else box[at] for f in state.fields.values()
            for box, at in odil.core.Domain._slots(f)]


def snapshot(states):
    """Per state its arrays (the objects) with a copy of their values."""
    return [[(a, a.detach().clone()) for a in _arrays(s)] for s in states]


def unchanged(states, before):
    """The states still hold the same array objects with the same values."""
    return all(len(_arrays(s)) == len(old) and all(now is a and torch.equal(now.detach(), copy)
                                                   for now, (a, copy) in zip(_arrays(s), old)) for s, old in zip(states, before))


def test_driver_refuses_members_by_name_before_tracing(cpu_mod, monkeypatch):
    def no_trace(*args, **kwargs):
        raise AssertionError("an operator was traced before the members were checked")

    monkeypatch.setattr(stencil_jit, "trace_outputs", no_trace)
    monkeypatch.setattr(stencil_jit, "trace", no_trace)
    monkeypatch.setattr(fused, "detect", no_trace)
    args = run_args()
    problems, states = make_members((16, 16), 3, np.float64, 3)

    def refused(problems, states, match, **kwargs):
        before = snapshot(states)
        with pytest.raises(ValueError, match=match):
            odil.util.optimize_ensemble(args, problems, states, **kwargs)
        assert unchanged(states, before)

    refused(problems, states[:2], "optimize_ensemble: 3 problems with 2 states", form="launches")
    # a differing cshape
    other = make_member((16, 32), 3, np.float64, 2, 3)
    refused(problems[:2] + [other[0]], states[:2] + [other[1]], "optimize_ensemble: member 2: level shapes .* differ from member 0's",
            form="launches")
    # a differing dtype
    other = make_member((16, 16), 3, np.float32, 1, 3)
    refused([problems[0], other[0]], [states[0], other[1]], "optimize_ensemble: member 1: dtype .* differ from member 0's", form="auto")
    # two unknowns
    two = make_member((16, 16), 3, np.float64, 1, 3)
    two[1].fields["w"] = two[0].domain.init_field(None)
    refused([problems[0], two[0]], [states[0], two[1]], "optimize_ensemble: member 1: 2 unknown fields", form="launches")
    # a network unknown
    net = make_member((16, 16), 3, np.float64, 1, 3)
    net[1].fields.clear()
    net[1].fields["u"] = net[0].domain.init_field(net[0].domain.make_neural_net([2, 4, 1]))
    refused([problems[0], net[0]], [states[0], net[1]],
            "optimize_ensemble: member 1: the unknown is not a cell-centred field of the domain", form="launches")
    # a 3-D member in the form of the 1-D / 2-D launches, and the other way round: no route admits them
    cube = make_members((8, 8, 8), 2, np.float64, 2)
    refused(*cube, "optimize_ensemble: member 0: 3-D grid: the batched launches run 1-D and 2-D grids", form="launches")
    refused(problems, states, "optimize_ensemble: member 0: 2-D grid: the batched launches of volumes run 3-D grids", form="volumes")
    # levels that the transfers do not take: one level of a MultigridField is a two-level rule for both routes
    flat = make_members((16, 16), 1, np.float64, 2)
    refused(*flat, "optimize_ensemble: member 0: 1 level", form="launches")


def test_driver_keeps_the_poisson_refusal_where_nothing_is_traced(cpu_mod, monkeypatch):
    """form='workgroup' (the default), or tracing switched off: a member that is not the Poisson stencil is refused with
    the text the Poisson ensembles always gave, whatever follows it."""
    monkeypatch.setattr(stencil_jit, "trace", lambda *a, **k: None)  # (no hipcc run for the single evaluator: not needed here)
    args = run_args()
    problems, states = make_members((16, 16), 3, np.float64, 2)
    before = snapshot(states)
    with pytest.raises(ValueError, match="optimize_ensemble: member 0: the operator is not the recognised Poisson stencil"):
        odil.util.optimize_ensemble(args, problems, states)
    with pytest.raises(ValueError, match="member 0: the operator is not the recognised Poisson stencil .*form='launches'"):
        odil.util.optimize_ensemble(args, problems, states, form="workgroup")
    monkeypatch.setattr(runtime, "enable_trace", False)
    problems, states2 = make_members((16, 16), 3, np.float64, 2)
    with pytest.raises(ValueError, match="member 0: the operator is not the recognised Poisson stencil .*ODIL_TRACE=0"):
        odil.util.optimize_ensemble(args, problems, states2, form="launches")
    assert unchanged(states, before)


def test_traced_refusal_exempts_one_level_and_follows_the_forms(cpu_mod):
    f64 = torch.float64
    assert fused.traced_refusal([(16, 16)], f64, "launches") is None  # (a plain Field: no transfers)
    assert fused.traced_refusal([(8, 8, 8)], f64, "volumes") is None
    assert "3-D" in fused.traced_refusal([(8, 8, 8)], f64, "launches")
    assert "4-D" in fused.traced_refusal([(4, 4, 4, 4)], f64, "launches")
    assert "float16" in fused.traced_refusal([(16, 16)], torch.float16, "launches")


# --------------------------------------------------------------------------------------------------------- 4: compile
@pytest.mark.parametrize("cshape,nlvl,beta,dtype", [((16, 16), 3, 1.0, np.float64), ((8, 8, 8), 2, 0.0, np.float32),
                                                    ((12, 18), 2, 1.0, np.float32)])
def test_batched_source_compiles_for_gfx950(cpu_mod, cshape, nlvl, beta, dtype):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc here: the batched source is not compiled")
    problem, state = make_member(cshape, nlvl, dtype, 0, 2, beta=beta)
    cg, source = generate(problem, state, True)
    lib, path = jit_cache._compile(source, cg.flags)
    assert os.path.exists(path)
    assert all(hasattr(lib, name) for name in ("jit_fwd", "jit_gather", "jit_fwd_batch", "jit_gather_batch"))
