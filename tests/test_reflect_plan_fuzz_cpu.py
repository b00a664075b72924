"""The planner's part of DSP_OP_REFLECTED_CONVOLVE on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/reflect_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the op with wild lengths, tap counts, slots, bindings, offsets
and strides, alone and with an avg_current behind it: each is planned -- on dsp_reflect_kernel, with an argument block whose bindings have
the right kind and size and which fits the kernel's LDS -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("reflect_plan_fuzz"), "reflect_plan_fuzz")


@pytest.mark.parametrize("seed", [0x19F, 4])
def test_programs_with_the_op_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # both shapes (the fused one with the filtered row stored and not) and both geometries were planned ...
    assert rep["plain"] > 1000 and rep["fused"] > 800 and 300 < rep["fused_row_stored"] < rep["fused"] - 300, rep
    assert rep["accepted"] == rep["plain"] + rep["fused"] == rep["narrow"] + rep["wide"] and rep["narrow"] > 300 and rep["wide"] > 1000, rep
    # ... and the refusals by name were reached: the shapes', the kernel longer than the rows, the limits'
    assert rep["refused_shape"] > 300 and rep["refused_long"] > 500 and rep["refused_limit"] > 500 and rep["refused_by_name"] > 3000, rep
