"""The planner's part of DSP_OP_LOG_CHECK, DSP_OP_POLY_FIT, DSP_OP_POLY_DIFF and DSP_OP_POLY_EXP_RMS on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/tailfit_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild lengths, numbers of coefficients, slots,
bindings, offsets and strides -- each processor alone, log_check -> poly_fit, the chain with its residuals, each with or without a
BL_SUBTRACT behind the LOAD --: each is planned -- on dsp_tailfit_kernel, with an argument block whose bindings have the right kind, type
and size and whose powers stay inside int64 -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("tailfit_plan_fuzz"), "tailfit_plan_fuzz")


@pytest.mark.parametrize("seed", [0x2F, 7])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every shape was planned: each processor alone, the fit behind the logarithm, the chain with either store or none, with a subtraction ...
    assert rep["log"] > 300 and rep["fit"] > 200 and rep["resid"] > 200 and rep["log_fit"] > 200 and rep["chain"] > 200, rep
    assert rep["accepted"] == rep["log"] + rep["fit"] + rep["resid"] + rep["log_fit"] + rep["chain"], rep
    assert 50 < rep["log_stored"] and 50 < rep["pars_stored"] < rep["chain"] - 50 and rep["subtracted"] > 200, rep
    # ... and the refusals by name were reached: the shapes', the number of coefficients', the powers'
    assert rep["refused_shape"] > 300 and rep["refused_many"] > 100 and rep["refused_power"] > 100 and rep["refused_by_name"] > 1500, rep
