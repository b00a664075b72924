"""The planner's part of DSP_OP_SVM_PREDICT on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with a
``main`` of its own, plain g++, no HIP, no LD_PRELOAD.

``tests/svm_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the op with wild row lengths, support-vector and class counts,
bindings, offsets and strides: each is planned -- on dsp_svm_kernel, with an argument block whose bindings have the right kind and size and
which fits the kernel's LDS and accumulators -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("svm_plan_fuzz"), "svm_plan_fuzz")


@pytest.mark.parametrize("seed", [0x19D, 3])
def test_programs_with_the_op_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # the shape was planned in both loops, with and without decisions, and refusals by name were reached: the shape's, the operands' and the limits'
    assert rep["accepted"] > 2000 and rep["with_decisions"] > 500 and rep["f64"] > 500 and rep["refused_by_name"] > 1000, rep
