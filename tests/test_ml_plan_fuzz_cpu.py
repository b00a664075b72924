"""The planner's part of DSP_OP_NORMALISE and DSP_OP_DENSE on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone
program with a ``main`` of its own, plain g++, no HIP, no LD_PRELOAD.

``tests/ml_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild activations, lengths, widths, slots, bindings,
offsets and strides: each is planned -- on dsp_dense_kernel, with an argument block whose bindings have the right kind and size and
which fits the kernel's LDS and accumulators -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("ml_plan_fuzz"), "ml_plan_fuzz")


@pytest.mark.parametrize("seed", [0x18D, 3])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every accepted shape was planned, fused and apart, and refusals by name were reached: the shapes', the operands' and the limits'
    assert rep["dense"] > 500 and rep["classify"] > 300 and rep["normalise"] > 300 and rep["fused"] > 300, rep
    assert rep["accepted"] == rep["dense"] + rep["classify"] + rep["normalise"] and rep["refused_by_name"] > 500, rep
