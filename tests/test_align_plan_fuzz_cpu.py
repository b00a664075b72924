"""The planner's part of DSP_OP_INL_CORRECTION, DSP_OP_WF_CENTROID, DSP_OP_WF_ALIGNMENT and DSP_OP_WF_CORRECTION on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/align_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild lengths, sizes, indices, slots, bindings, offsets
and strides -- each processor alone, wf_alignment -> wf_correction with the aligned row stored or not --: each is planned -- in one of the five
shapes, on dsp_align_kernel, with an argument block whose lengths, indices and bindings are in range -- or refused with a reason.  The rule of
a window (dsp_align_window, which the kernel runs per row) is held inside the row for every centroid, shift and size beside it."""
import pytest

from plan_fuzz_util import build, run


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("align_plan_fuzz"), "align_plan_fuzz")


@pytest.mark.parametrize("seed", [0x2F, 7])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every shape was planned: each processor alone, the pair with the aligned row stored and without, a centroid per event, integer rows ...
    assert min(rep["inl"], rep["centroid"], rep["align"], rep["correct"], rep["fused"]) > 200, rep
    assert rep["accepted"] == rep["inl"] + rep["centroid"] + rep["align"] + rep["correct"] + rep["fused"], rep
    assert 50 < rep["aligned_stored"] < rep["fused"] - 50 and rep["per_event"] > 200 and rep["integer_rows"] > 500, rep
    # ... and the refusals by name were reached: the shapes', the reference's checks'
    assert rep["refused_shape"] > 300 and rep["refused_check"] > 300 and rep["refused_by_name"] > 1500, rep
