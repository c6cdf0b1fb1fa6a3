"""Host checks of the ensembles of inverse problems with `NeuralNet` unknowns and outputs in parameter space
(`odil.util.optimize_ensemble`: `_Codegen(batch="params")`, `k_par_batch`, `stencil_bind.EpochBatch`), no GPU:

1  generator, networks: for heat with --kwreg at the fixture's arguments the batched kernels are the single bodies under the
   member head, `k_par_batch` is the body of `k_par`, `k_final_batch` runs on nout + 46 rows; batch=True keeps its refusal
2  generator, other operators: batch=True keeps "outputs in parameter space"; an operator without networks and without
   such outputs gives the same bytes with True and "params"; batch=False is what it was
3  the batched sources build for gfx950 and export `jit_par_batch` (where hipcc is present: a compile, nothing more)
4  the driver's refusals name the member before anything is traced and leave the states alone; the pinned texts stay

Operators are traced on CPU tensors; the comparison helpers are those of tests/test_traced_ensemble_host.py."""

import os
import shutil

import numpy as np
import pytest
from net_ensemble_members import generate, make_member, make_members, run_args
from test_traced_ensemble_host import body_after_head, cpu_mod, kernel_lines, snapshot, unchanged  # noqa: F401
from test_traced_ensemble_host import generate as generate_plain

import odil_amd as odil
from odil_amd import fused, jit_cache, stencil_bind, stencil_jit
from odil_amd.stencil_trace import TraceUnsupported

NPAR = 46  # the parameters of a [1, 5, 5, 1] network: 5 + 25 + 5 weights, 5 + 5 + 1 biases


def par_body_after_head(many):
    """The lines of `k_par_batch` behind its head: the member's `Args` (what `body_after_head` strips) and `ParArgs`."""
    rest = body_after_head(many, "blockIdx.x")
    assert rest[0] == "  ParArgs pa;" and rest[1] == "  __builtin_memcpy(&pa, (ParArgsC*)(pb + blockIdx.x), sizeof(ParArgs));"
    return rest[2:]


# ---------------------------------------------------------------------------------------------- 1: generator, networks
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batched_kernels_of_heat_share_the_single_bodies(cpu_mod, dtype):
    problem, state = make_member("heat", dtype, 0)
    cg1, single = generate(problem, state, False)
    cg2, batch = generate(problem, state, "params")
    assert "_batch" not in single
    assert cg2.nets == [("k_net", (1, 5, 5, 1))] and not cg2.arrays and len(cg2.pg_decl) == NPAR and cg1.pg_decl == cg2.pg_decl
    assert cg2.wregs == "mem" and "#define W(s, l, k) a.par[WOFS_##s##_##l][k]" in batch
    assert cg1.gathers == cg2.gathers and cg1.direct == cg2.direct and cg1.fwd_blocks == cg2.fwd_blocks
    nout = len(cg2.outputs)
    assert nout == 4 and [k for k, _ in cg2.par_outputs] == [4]  # fu, imp, xreg, treg on the grid; wreg in parameter space
    for name, member in [("k_fwd", "blockIdx.y"), ("k_final", "blockIdx.z"), ("k_loss", "blockIdx.x")] + [
            ("k_gat_{}".format(gi), "blockIdx.y") for gi in range(len(cg2.gathers))]:
        one = kernel_lines(single, name)
        assert kernel_lines(batch, name) == one, "{} of the batched source differs".format(name)
        many = kernel_lines(batch, name + "_batch")
        assert body_after_head(many, member) == one[1:], "the bodies of {} differ".format(name)
        assert not any(member in line for line in one)
    one = kernel_lines(single, "k_par")
    assert kernel_lines(batch, "k_par") == one
    many = kernel_lines(batch, "k_par_batch")
    assert many[0] == ('extern "C" __global__ __launch_bounds__(NB) void k_par_batch(const Args* __restrict__ ab, '
                       'const ParArgs* __restrict__ pb) {')
    assert par_body_after_head(many) == one[1:]
    assert not any("blockIdx" in line for line in one)  # (one workgroup: the member is blockIdx.x)
    assert any("HS(" in line for line in one)  # (the annealed weight travels as a host scalar of the member's block)
    # the launchers
    assert "k_final, dim3({}, SEG)".format(nout + NPAR) in batch
    assert "k_final_batch, dim3({}, SEG, nmembers)".format(nout + NPAR) in batch
    assert 'extern "C" int jit_par_batch(const void* args_dev, const void* pargs_dev, int nmembers, void* stream) {' in batch
    assert "k_par_batch, dim3(nmembers), dim3(NB)" in batch
    assert batch.count("if (nmembers < 1 || nmembers > 65535) return -1;") == 3
    assert "jit_par_batch" in stencil_bind._ARGTYPES
    # batch=True is what it was: the refusal of networks
    with pytest.raises(TraceUnsupported, match="network or Array parameters"):
        generate(problem, state, True)


def test_live_operator_has_rows_for_the_network_and_the_array(cpu_mod):
    """u, k_net, c: `a.par` holds the network's six arrays, then the Array (`AP` behind them); 46 + 4 rows."""
    problem, state = make_member("heat", np.float64, 0, operator="live")
    cg, batch = generate(problem, state, "params")
    assert cg.nets == [("k_net", (1, 5, 5, 1))] and cg.arrays == [("c", 4)] and len(cg.pg_decl) == NPAR + 4
    assert "#define AP(s, k) a.par[6 + s][k]" in batch and cg.par_arrays == 7
    assert [k for k, _ in cg.par_outputs] == [4, 5, 6] and cg.par_index == [3, 4, 5, 6, 7, 8, 9]
    assert "k_final_batch, dim3({}, SEG, nmembers)".format(4 + NPAR + 4) in batch
    # a network read only with frozen=True: no rows, its gradient slots are SET by the parameter kernel
    problem, state = make_member("heat", np.float64, 0, operator="frozen")
    cg, batch = generate(problem, state, "params")
    assert cg.nets and not cg.pg_decl and "k_net" not in cg.pgrads
    par = kernel_lines(batch, "k_par_batch")
    assert sum("pa.grad[" in line for line in par) == 6 and not any("= pa.grad[" in line for line in par)


# ---------------------------------------------------------------------------------------- 2: generator, other operators
def test_true_keeps_its_refusals_and_members_without_parameters_their_bytes(cpu_mod):
    domain = odil.Domain(cshape=(8, 8), dtype=np.float64)
    pstate = odil.State()
    pstate.fields["u"] = odil.Field(None, loc="cc")
    pstate.fields["p"] = odil.Array(np.array([1.0, -2.0, 0.5]))
    pstate = domain.init_state(pstate)
    op = lambda ctx: [ctx.field("u") - ctx.field("u", 1, 0), ctx.domain.arrays_from_field(ctx.state.fields["p"])[0] * 2.0]
    with pytest.raises(TraceUnsupported, match="outputs in parameter space"):
        stencil_jit.TracedOperator(odil.Problem(op, domain), pstate, batch=True)
    # a diffusion member: no networks, no outputs in parameter space
    from traced_ensemble_members import make_member as diffusion_member

    problem, state = diffusion_member((16, 16), 3, np.float64, 0, 2, beta=1.0)
    before = generate_plain(problem, state, False)[1]
    with_true = generate_plain(problem, state, True)[1]
    with_params = generate_plain(problem, state, "params")[1]
    assert with_params == with_true and "k_par" not in with_params
    assert generate_plain(problem, state, False)[1] == before and "_batch" not in before
    # ... and heat's single source is unchanged by a batched generation before it
    problem, state = make_member("heat", np.float64, 0)
    single = generate(problem, state, False)[1]
    generate(problem, state, "params")
    assert generate(problem, state, False)[1] == single


# --------------------------------------------------------------------------------------------------------- 3: compile
@pytest.mark.parametrize("which,dtype", [("heat", np.float64), ("heat2d", np.float32)])
def test_batched_source_with_a_network_compiles_for_gfx950(cpu_mod, which, dtype):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc here: the batched source is not compiled")
    problem, state = make_member(which, dtype, 0, operator="heat" if which == "heat" else "live")
    cg, source = generate(problem, state, "params")
    lib, path = jit_cache._compile(source, cg.flags)
    assert os.path.exists(path)
    assert all(hasattr(lib, name) for name in ("jit_fwd", "jit_par", "jit_fwd_batch", "jit_gather_batch", "jit_par_batch"))


# ---------------------------------------------------------------------------------------------- 4: the driver's refusals
def test_driver_refuses_networks_that_differ_before_tracing(cpu_mod, monkeypatch):
    def no_trace(*args, **kwargs):
        raise AssertionError("an operator was traced before the members were checked")

    monkeypatch.setattr(stencil_jit, "trace_outputs", no_trace)
    monkeypatch.setattr(stencil_jit, "trace", no_trace)
    monkeypatch.setattr(fused, "detect", no_trace)
    problems, states = make_members("heat", np.float64, 3, operator="live")

    def refused(problems, states, match, args=run_args(), **kwargs):
        before = snapshot(states)
        with pytest.raises(ValueError, match=match):
            odil.util.optimize_ensemble(args, problems, states, **kwargs)
        assert unchanged(states, before)

    # differing layer shapes
    other = make_member("heat", np.float64, 1, operator="live", arch=(5, 4))
    refused([problems[0], other[0]], [states[0], other[1]],
            r"optimize_ensemble: member 1: NeuralNet unknowns \(key, position in the state, layer shapes\) .*\(4, 5\).* "
            r"differ from member 0's", form="launches")
    # a network missing in member 2
    hproblems, hstates = make_members("heat", np.float64, 2)
    bare = make_member("heat", np.float64, 2)
    del bare[1].fields["k_net"]
    refused(hproblems + [bare[0]], hstates + [bare[1]],
            r"optimize_ensemble: member 2: NeuralNet unknowns \(key, position in the state, layer shapes\) \[\] differ from member 0's",
            form="auto")
    # another position, and another key of the Array beside it
    moved = make_member("heat", np.float64, 1, operator="live", order="before")
    refused([problems[0], moved[0]], [states[0], moved[1]], "member 1: Array unknowns .* differ from member 0's", form="launches")
    renamed = make_member("heat", np.float64, 1, operator="live")
    renamed[1].fields["c2"] = renamed[1].fields.pop("c")
    refused([problems[0], renamed[0]], [states[0], renamed[1]], "member 1: Array unknowns .*'c2'.* differ from member 0's", form="launches")
    # the pinned texts: a network under a key where member 0 has none counts as a second field ...
    renamed = make_member("heat", np.float64, 1, operator="live")
    renamed[1].fields["k2"] = renamed[1].fields.pop("k_net")
    refused([problems[0], renamed[0]], [states[0], renamed[1]], "optimize_ensemble: member 1: 2 unknown fields", form="launches")
    from param_ensemble_members import make_member as array_member

    plain = array_member((16, 24), 3, np.float64, 0)
    net = array_member((16, 24), 3, np.float64, 1)
    net[1].fields["net"] = net[0].domain.init_field(net[0].domain.make_neural_net([2, 4, 1]))
    refused([plain[0], net[0]], [plain[1], net[1]], "optimize_ensemble: member 1: 2 unknown fields", form="launches")
    # ... and a member whose only field is a network is no cell-centred field
    alone = array_member((16, 24), 3, np.float64, 1)
    alone[1].fields.clear()
    alone[1].fields["u"] = alone[0].domain.init_field(alone[0].domain.make_neural_net([2, 4, 1]))
    refused([alone[0]], [alone[1]], "member 0: the unknown is not a cell-centred field of the domain", form="launches")
    # members that agree pass the structural checks; here (CPU tensors) no route runs them, and the refusal says which would
    refused(problems, states, "member 0: 1 Array unknown and 1 NeuralNet unknown beside the field: such members run as traced "
            "operators", form="launches")
    refused(problems, states, "member 0: 1 Array unknown and 1 NeuralNet unknown beside the field", form="workgroup")
    refused(*make_members("heat", np.float64, 2), "member 0: 1 NeuralNet unknown beside the field",
            args=run_args("lbfgsb", epochs=12), form="auto")


def test_newton_ensemble_keeps_refusing_network_unknowns(cpu_mod):
    problems, states = make_members("plain", np.float64, 2)
    before = snapshot(states)
    args = run_args("newton", epochs=2, linsolver="direct")
    with pytest.raises(ValueError, match="optimize_newton_ensemble: member 0: 2 unknown fields"):
        odil.util.optimize_newton_ensemble(args, problems, states)
    assert unchanged(states, before)
