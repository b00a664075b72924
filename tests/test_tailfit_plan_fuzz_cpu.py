"""The planner's part of DSP_OP_LOG_CHECK, DSP_OP_POLY_FIT, DSP_OP_POLY_DIFF and DSP_OP_POLY_EXP_RMS on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/tailfit_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild lengths, numbers of coefficients, slots,
bindings, offsets and strides -- each processor alone, log_check -> poly_fit, the chain with its residuals, each with or without a
BL_SUBTRACT behind the LOAD --: each is planned -- on dsp_tailfit_kernel, with an argument block whose bindings have the right kind, type
and size and whose powers stay inside int64 -- or refused with a reason."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspeed_amd", "csrc")
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")
    exe = str(tmp_path_factory.mktemp("tailfit_plan_fuzz") / "tailfit_plan_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "tailfit_plan_fuzz.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    return exe


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("DSPEED_HIP_"):
            del env[k]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [0x2F, 7])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = _run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every shape was planned: each processor alone, the fit behind the logarithm, the chain with either store or none, with a subtraction ...
    assert rep["log"] > 300 and rep["fit"] > 200 and rep["resid"] > 200 and rep["log_fit"] > 200 and rep["chain"] > 200, rep
    assert rep["accepted"] == rep["log"] + rep["fit"] + rep["resid"] + rep["log_fit"] + rep["chain"], rep
    assert 50 < rep["log_stored"] and 50 < rep["pars_stored"] < rep["chain"] - 50 and rep["subtracted"] > 200, rep
    # ... and the refusals by name were reached: the shapes', the number of coefficients', the powers'
    assert rep["refused_shape"] > 300 and rep["refused_many"] > 100 and rep["refused_power"] > 100 and rep["refused_by_name"] > 1500, rep
