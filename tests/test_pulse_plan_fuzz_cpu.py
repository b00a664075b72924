"""The planner's part of DSP_OP_PEAK_SNR_THRESHOLD and DSP_OP_MULTI_A_FILTER on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/pulse_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild lengths, list lengths, slots, bindings, offsets,
strides and operands -- the picker alone, the pick-off alone, both in one launch with the packed list stored or not --: each is planned -- on
dsp_pulses_kernel, with an argument block whose bindings have the right kind, type and size and whose list, width and lengths keep the
kernel's bounds -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pulse_plan_fuzz"), "pulse_plan_fuzz")


@pytest.mark.parametrize("seed", [0x31, 9])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every shape was planned: the picker, the pick-off, both in one launch with the packed list stored and not, the ratio a column ...
    assert rep["picker"] > 500 and rep["pickoff"] > 500 and rep["fused"] > 500 and 100 < rep["fused_list_stored"] < rep["fused"] - 100, rep
    assert rep["accepted"] == rep["picker"] + rep["pickoff"] + rep["fused"] and rep["ratio_columns"] > 200, rep
    # ... and the refusals by name were reached: the shapes', the long lists', the width's, the outputs' lengths, the pick-off's return array
    assert rep["refused_shape"] > 300 and rep["refused_long"] > 100 and rep["refused_width"] > 100 and rep["refused_lengths"] > 300, rep
    assert rep["refused_return"] > 50 and rep["refused_by_name"] > 2000, rep
