"""Host checks of the ensembles of inverse problems (`odil.util.optimize_ensemble` for members with `Array` unknowns beside
their field: `fused.TracedLaunchEnsemble`, `stencil_bind.EpochBatch`), no GPU:

1  generator: for a member with `u` + `Array(3)` the batched kernels are the single bodies under the member head, and the
   launcher runs `k_final_batch` on nout + npg rows; networks keep their refusal
2  the batched source builds for gfx950 (where hipcc is present: a compile, nothing more)
3  the driver's new refusals name the member and leave the states alone; the Newton driver keeps refusing such members

Operators are traced on CPU tensors; the comparison helpers are those of tests/test_traced_ensemble_host.py."""

import os
import shutil

import numpy as np
import pytest
from param_ensemble_members import make_member, make_members, run_args
from test_traced_ensemble_host import body_after_head, cpu_mod, generate, kernel_lines, snapshot, unchanged  # noqa: F401

import odil_amd as odil
from odil_amd import fused, jit_cache, stencil_jit

CASES = [((64,), 3, "after"), ((16, 24), 3, "before"), ((12, 18), None, "after"), ((8, 8, 16), 2, "after")]


# ------------------------------------------------------------------------------------------------------- 1: generator
@pytest.mark.parametrize("cshape,nlvl,order", CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batched_kernels_of_a_member_with_an_array_share_the_single_bodies(cpu_mod, cshape, nlvl, order, dtype):
    problem, state = make_member(cshape, nlvl, dtype, 0, order=order)
    cg1, single = generate(problem, state, False)
    cg2, batch = generate(problem, state, True)
    assert "_batch" not in single
    assert cg2.arrays == [("coeff", 3)] and len(cg2.pg_decl) == 3 and cg1.pg_decl == cg2.pg_decl and not cg2.nets
    assert cg1.gathers == cg2.gathers and cg1.direct == cg2.direct and cg1.fwd_blocks == cg2.fwd_blocks
    nout, npg = len(cg2.outputs), len(cg2.pg_decl)
    assert nout == 2
    for name, member in [("k_fwd", "blockIdx.y"), ("k_final", "blockIdx.z"), ("k_loss", "blockIdx.x")] + [
            ("k_gat_{}".format(gi), "blockIdx.y") for gi in range(len(cg2.gathers))]:
        one = kernel_lines(single, name)
        assert kernel_lines(batch, name) == one, "{} of the batched source differs".format(name)
        many = kernel_lines(batch, name + "_batch")
        assert body_after_head(many, member) == one[1:], "the bodies of {} differ".format(name)
        assert not any(member in line for line in one)
    # the member's own argument block carries its constants, partial sums and parameter gradients
    fwd, loss = kernel_lines(batch, "k_fwd_batch"), kernel_lines(batch, "k_loss_batch")
    assert any("AP(0, " in line for line in fwd) and "#define AP(s, k) a.par[0 + s][k]" in batch
    assert sum("a.ppart[" in line for line in fwd) == npg
    assert any("a.pgrad[k - {}] = s;".format(nout) in line for line in loss)
    # the launchers: k_final over the rows of the outputs AND of the parameter gradients, in the single launch and the batched
    assert "k_final, dim3({}, SEG)".format(nout + npg) in batch
    assert "k_final_batch, dim3({}, SEG, nmembers)".format(nout + npg) in batch
    assert "k_loss_batch, dim3(nmembers), dim3(64)" in batch


def test_two_arrays_give_rows_in_the_order_they_are_read(cpu_mod):
    """`coeff` (3,) and `mix` (2, 2), of which the operator reads [0, 1] and [1, 0]: seven rows, every element of an Array
    that is read has one, at `pg_offset` of its Array plus its position in the contiguous array."""
    problem, state = make_member((16, 24), 3, np.float64, 0, order="around", mix=True)
    cg, batch = generate(problem, state, True)
    assert sorted(cg.arrays) == [("coeff", 3), ("mix", 4)] and len(cg.pg_decl) == 7
    assert set(cg.pg_offset) == {"coeff", "mix"} and sorted(cg.pg_offset.values()) in ([0, 3], [0, 4])
    slot = dict((key, k) for k, (key, _) in enumerate(cg.arrays))["mix"]
    assert "AP({}, 1)".format(slot) in batch and "AP({}, 2)".format(slot) in batch
    assert "AP({}, 0)".format(slot) not in batch and "AP({}, 3)".format(slot) not in batch
    assert "k_final_batch, dim3(9, SEG, nmembers)" in batch


def test_networks_keep_their_refusal(cpu_mod, monkeypatch):
    import sys

    from conftest import ROOT
    from odil_amd.stencil_trace import TraceUnsupported

    sys.path.insert(0, os.path.join(ROOT, "examples", "heat"))
    import heat2d

    hargs = ["--Nt", "8", "--Nx", "16", "--Ny", "128", "--infer_k", "1", "--imposed", "stripe", "--multigrid", "0"]
    monkeypatch.setenv("ODIL_TRACE_SHARE", "0")
    with pytest.raises(TraceUnsupported, match="network or Array parameters"):
        generate(*heat2d.make_problem(heat2d.parse_args(hargs)), True)


# --------------------------------------------------------------------------------------------------------- 2: compile
@pytest.mark.parametrize("cshape,nlvl,dtype", [((16, 24), 3, np.float64), ((8, 8, 16), 2, np.float32)])
def test_batched_source_with_an_array_compiles_for_gfx950(cpu_mod, cshape, nlvl, dtype):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc here: the batched source is not compiled")
    problem, state = make_member(cshape, nlvl, dtype, 0)
    cg, source = generate(problem, state, True)
    lib, path = jit_cache._compile(source, cg.flags)
    assert os.path.exists(path)
    assert all(hasattr(lib, name) for name in ("jit_fwd", "jit_gather", "jit_fwd_batch", "jit_gather_batch"))


# ---------------------------------------------------------------------------------------------- 3: the driver's refusals
def test_driver_refuses_arrays_that_differ_before_tracing(cpu_mod, monkeypatch):
    def no_trace(*args, **kwargs):
        raise AssertionError("an operator was traced before the members were checked")

    monkeypatch.setattr(stencil_jit, "trace_outputs", no_trace)
    monkeypatch.setattr(stencil_jit, "trace", no_trace)
    monkeypatch.setattr(fused, "detect", no_trace)
    # (members on CPU tensors: nothing is traceable, so every member that passes the structural checks is refused by the
    # route -- AFTER the checks of the members among each other)
    problems, states = make_members((16, 24), 3, np.float64, 3)

    def refused(problems, states, match, args=run_args(), **kwargs):
        before = snapshot(states)
        with pytest.raises(ValueError, match=match):
            odil.util.optimize_ensemble(args, problems, states, **kwargs)
        assert unchanged(states, before)

    # a differing Array shape
    other = make_member((16, 24), 3, np.float64, 1, coeff_shape=(4,))
    refused([problems[0], other[0]], [states[0], other[1]],
            r"optimize_ensemble: member 1: Array unknowns \(key, position in the state, shape\) .*\(4,\).* differ from member 0's",
            form="launches")
    # a missing key: the member is a forward problem among inverse problems
    from param_ensemble_members import forward_only

    bare = make_member((16, 24), 3, np.float64, 2, operator_=forward_only)
    refused(problems[:2] + [bare[0]], states[:2] + [bare[1]],
            r"optimize_ensemble: member 2: Array unknowns \(key, position in the state, shape\) \[\] differ from member 0's",
            form="auto")
    # another key, another position
    renamed = make_member((16, 24), 3, np.float64, 1)
    renamed[1].fields["c"] = renamed[1].fields.pop("coeff")
    refused([problems[0], renamed[0]], [states[0], renamed[1]], "member 1: Array unknowns .*'c'.* differ from member 0's", form="launches")
    moved = make_member((16, 24), 3, np.float64, 1, order="before")
    refused([problems[0], moved[0]], [states[0], moved[1]], "member 1: Array unknowns .* differ from member 0's", form="launches")
    # the refusals that were there keep their texts: two grid fields, a network beside the field, a network alone
    two = make_member((16, 24), 3, np.float64, 1)
    two[1].fields["w"] = two[0].domain.init_field(None)
    refused([problems[0], two[0]], [states[0], two[1]], "optimize_ensemble: member 1: 2 unknown fields", form="launches")
    net = make_member((16, 24), 3, np.float64, 1)
    net[1].fields["net"] = net[0].domain.init_field(net[0].domain.make_neural_net([2, 4, 1]))
    refused([problems[0], net[0]], [states[0], net[1]], "optimize_ensemble: member 1: 2 unknown fields", form="launches")
    alone = make_member((16, 24), 3, np.float64, 1)
    alone[1].fields.clear()
    alone[1].fields["u"] = alone[0].domain.init_field(alone[0].domain.make_neural_net([2, 4, 1]))
    refused([alone[0]], [alone[1]], "member 0: the unknown is not a cell-centred field of the domain", form="launches")
    # members that agree pass the structural checks; here (CPU tensors) no route runs them, and the refusal says which would
    refused(problems, states, "member 0: 1 Array unknown beside the field: such members run as traced operators", form="launches")
    refused(problems, states, "member 0: 1 Array unknown beside the field", form="workgroup")
    refused(problems, states, "member 0: 1 Array unknown beside the field", args=run_args("lbfgsb", epochs=12), form="auto")


def test_newton_ensemble_keeps_refusing_array_unknowns(cpu_mod):
    problems, states = make_members((16, 24), None, np.float64, 2)
    before = snapshot(states)
    args = run_args("newton", epochs=2, linsolver="direct")
    with pytest.raises(ValueError, match="optimize_newton_ensemble: member 0: 2 unknown fields"):
        odil.util.optimize_newton_ensemble(args, problems, states)
    assert unchanged(states, before)
