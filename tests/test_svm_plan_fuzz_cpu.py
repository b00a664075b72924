"""The planner's part of DSP_OP_SVM_PREDICT on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program with a
``main`` of its own, plain g++, no HIP, no LD_PRELOAD.

``tests/svm_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the op with wild row lengths, support-vector and class counts,
bindings, offsets and strides: each is planned -- on dsp_svm_kernel, with an argument block whose bindings have the right kind and size and
which fits the kernel's LDS and accumulators -- or refused with a reason."""
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
    exe = str(tmp_path_factory.mktemp("svm_plan_fuzz") / "svm_plan_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "svm_plan_fuzz.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    return exe


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("DSPEED_HIP_"):
            del env[k]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [0x19D, 3])
def test_programs_with_the_op_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = _run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # the shape was planned in both loops, with and without decisions, and refusals by name were reached: the shape's, the operands' and the limits'
    assert rep["accepted"] > 2000 and rep["with_decisions"] > 500 and rep["f64"] > 500 and rep["refused_by_name"] > 1000, rep
