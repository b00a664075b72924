"""The planner's part of DSP_OP_RC_CR2 and DSP_OP_BI_LEVEL_ZERO_CROSSING on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/pileup_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild lengths, list lengths, slots, bindings, offsets,
strides and operands -- the filter alone, the walk alone, both in one launch, each with or without a BL_SUBTRACT behind the LOAD --: each is
planned -- on dsp_pileup_kernel, with an argument block whose bindings have the right kind, type and size -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pileup_plan_fuzz"), "pileup_plan_fuzz")


@pytest.mark.parametrize("seed", [0x2F, 7])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every shape was planned: the filter, the walk, both in one launch with the filtered row stored and not, with a subtraction, with columns ...
    assert rep["filter"] > 500 and rep["walk"] > 300 and rep["fused"] > 300 and 100 < rep["fused_row_stored"] < rep["fused"] - 100, rep
    assert rep["accepted"] == rep["filter"] + rep["walk"] + rep["fused"] and rep["subtracted"] > 200 and rep["columns"] > 300, rep
    # ... and the refusals by name were reached: the shapes', the short rows', t_start's, the lists'
    assert rep["refused_shape"] > 300 and rep["refused_short"] > 20 and rep["refused_start"] > 100 and rep["refused_lists"] > 300 and rep["refused_by_name"] > 2000, rep
