"""Host checks of the ensembles whose members have several grid unknowns or node-centred axes (`odil.util.optimize_ensemble`
on the traced route: `fused.TracedLaunchEnsemble` with stacked rows), no GPU:

1  generator: the batched sources of `pair` ('cc', 'nc') and of `tracer` hold the single bodies under the member head
2  the driver's new refusals name the member and leave the states alone; the Newton driver keeps `2 unknown fields`
3  `fused.traced_refusal` asks the library about stacked rows (odil_mg_members_levels_ok)

Operators are traced on CPU tensors; the comparison helpers are those of tests/test_traced_ensemble_host.py."""

import numpy as np
import pytest
import torch
from fields_ensemble_members import pair, run_args, tracer
from test_traced_ensemble_host import body_after_head, cpu_mod, generate, kernel_lines, snapshot, unchanged  # noqa: F401

import odil_amd as odil
from odil_amd import fused, stencil_jit

BUILD = dict([
    ("pair-cc", lambda dtype: pair((16, 24), "cc", 3, dtype, 0)),
    ("pair-nc", lambda dtype: pair((8, 16), "nc", 3, dtype, 0)),
    ("tracer", lambda dtype: tracer(2, dtype, 0)),
    ("tracer-plain", lambda dtype: tracer(None, dtype, 0)),
])


# ------------------------------------------------------------------------------------------------------- 1: generator
@pytest.mark.parametrize("case", list(BUILD))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_batched_kernels_of_several_fields_share_the_single_bodies(cpu_mod, case, dtype):
    problem, state = BUILD[case](dtype)
    cg1, single = generate(problem, state, False)
    cg2, batch = generate(problem, state, "params")
    assert "_batch" not in single and "k_fwd_batch" in batch
    assert cg1.gathers == cg2.gathers and cg1.direct == cg2.direct and cg1.merged == cg2.merged
    assert len(cg2.src_keys) == len(state.fields) and set(cg2.src_keys) == set(state.fields)
    if case.startswith("tracer"):
        assert tuple(cg2.G) == (5, 8, 16) and cg2.merged == ["vx", "vy", "u"]
    elif case == "pair-nc":
        assert tuple(cg2.G) == (9, 16)
    names = [("k_fwd", "blockIdx.y"), ("k_final", "blockIdx.z"), ("k_loss", "blockIdx.x")]
    names += [("k_gat_all", "blockIdx.y")] if cg2.merged else []
    names += [("k_gat_{}".format(gi), "blockIdx.y") for gi, key in enumerate(cg2.gathers) if key not in cg2.merged]
    for name, member in names:
        one = kernel_lines(single, name)
        assert kernel_lines(batch, name) == one, "{} of the batched source differs".format(name)
        many = kernel_lines(batch, name + "_batch")
        assert body_after_head(many, member) == one[1:], "the bodies of {} differ".format(name)
        assert not any(member in line for line in one)


# ---------------------------------------------------------------------------------------------- 2: the driver's refusals
def test_driver_refuses_members_by_name_before_tracing(cpu_mod, monkeypatch):
    def no_trace(*args, **kwargs):
        raise AssertionError("an operator was traced before the members were checked")

    monkeypatch.setattr(stencil_jit, "trace_outputs", no_trace)
    monkeypatch.setattr(stencil_jit, "trace", no_trace)
    monkeypatch.setattr(fused, "detect", no_trace)
    args = run_args()
    f64 = np.float64

    def refused(built, match, **kwargs):
        problems, states = [p for p, _ in built], [s for _, s in built]
        before = snapshot(states)
        with pytest.raises(ValueError, match=match):
            odil.util.optimize_ensemble(args, problems, states, **kwargs)
        assert unchanged(states, before)

    good = lambda b: pair((8, 16), "nc", 3, f64, b)
    # fields at two locations
    refused([good(0), pair((8, 16), "nc", 3, f64, 1, locs=dict(w="cc"))],
            "optimize_ensemble: member 1: grid unknowns at two locations: 'u' at 'nc', 'w' at 'cc'", form="launches")
    # fields of two kinds
    refused([good(0), pair((8, 16), "nc", 3, f64, 1, kinds=dict(w="plain"))],
            "optimize_ensemble: member 1: grid unknowns of two kinds: 'u' is a MultigridField, 'w' a Field", form="launches")
    # a member with another key order
    refused([good(0), pair((8, 16), "nc", 3, f64, 1, keys=("w", "u"))],
            "optimize_ensemble: member 1: grid unknowns .*'w', 0.* differ from member 0's", form="launches")
    # another number of fields keeps the pinned text
    three = good(1)
    three[1].fields["z"] = three[0].domain.init_field(odil.Field(None, loc="nc"))
    refused([good(0), three], "optimize_ensemble: member 1: 3 unknown fields", form="launches")
    # 'nn' members of 9 x 9 = 81 elements lie back to back off the 16-byte grid
    refused([pair((8, 8), "nn", None, f64, b) for b in range(2)],
            "optimize_ensemble: member 0: a member of 81 cells is not a multiple of 16 bytes", form="launches")
    # a 4-D member
    refused([pair((4, 4, 4, 8), "nccc", None, f64, b) for b in range(2)],
            "optimize_ensemble: member 0: 4-D grid: the batched launches of traced operators run 1-D to 3-D grids", form="auto")
    # the form that runs whole epochs in one workgroup, and members on the host: the traced route alone serves such members
    refused([good(b) for b in range(2)], "optimize_ensemble: member 0: 2 grid unknowns: such members run as traced operators")
    refused([good(b) for b in range(2)], "optimize_ensemble: member 0: 2 grid unknowns: such members run as traced operators",
            form="launches")


def test_newton_driver_keeps_refusing_two_fields(cpu_mod):
    built = [pair((8, 16), "cc", None, np.float64, b) for b in range(2)]
    problems, states = [p for p, _ in built], [s for _, s in built]
    before = snapshot(states)
    with pytest.raises(ValueError, match="optimize_newton_ensemble: member 0: 2 unknown fields"):
        odil.util.optimize_newton_ensemble(run_args("newton", epochs=2, linsolver="direct"), problems, states)
    assert unchanged(states, before)


# ------------------------------------------------------------------------------------------------------- 3: the library
def test_traced_refusal_asks_the_library_about_stacked_rows(cpu_mod):
    f64, f32 = torch.float64, torch.float32
    nc = [(9, 16), (5, 8), (3, 4)]
    assert fused.traced_refusal(nc, f64, "launches", 5, loc="nc", nfields=2) is None
    assert fused.traced_refusal([(16, 9), (8, 5), (4, 3)], f32, "launches", 5, loc="cn", nfields=1) is None
    assert fused.traced_refusal([(5, 8, 16), (3, 4, 8)], f32, "volumes", 5, loc="ncc", nfields=3) is None
    assert "3-D" in fused.traced_refusal([(5, 8, 16), (3, 4, 8)], f64, "launches", 5, loc="ncc", nfields=3)
    assert "rows (1 ... 65535)" in fused.traced_refusal(nc, f64, "launches", 35000, loc="nc", nfields=2)
    assert "does not refine" in fused.traced_refusal([(9, 16), (5, 7)], f64, "launches", 2, loc="nc", nfields=2)
    # a time axis long enough for the node-centred marching kernel of a single run: it runs row by row
    assert fused.traced_refusal([(17, 64, 64), (9, 32, 32)], f64, "volumes", 4, loc="ncc", nfields=3) is None
    # one cell-centred unknown keeps the answers of the forms
    assert fused.traced_refusal([(16, 24), (8, 12)], f64, "launches", 3, loc="cc", nfields=1) is None
    assert fused.traced_refusal([(16, 16)], f64, "launches", loc="cc") is None
