"""The planner's part of DSP_OP_NORMALISE and DSP_OP_DENSE on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone
program with a ``main`` of its own, plain g++, no HIP, no LD_PRELOAD.

``tests/ml_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild activations, lengths, widths, slots, bindings,
offsets and strides: each is planned -- on dsp_dense_kernel, with an argument block whose bindings have the right kind and size and
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
    exe = str(tmp_path_factory.mktemp("ml_plan_fuzz") / "ml_plan_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "ml_plan_fuzz.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    return exe


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("DSPEED_HIP_"):
            del env[k]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [0x18D, 3])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = _run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every accepted shape was planned, fused and apart, and refusals by name were reached: the shapes', the operands' and the limits'
    assert rep["dense"] > 500 and rep["classify"] > 300 and rep["normalise"] > 300 and rep["fused"] > 300, rep
    assert rep["accepted"] == rep["dense"] + rep["classify"] + rep["normalise"] and rep["refused_by_name"] > 500, rep
