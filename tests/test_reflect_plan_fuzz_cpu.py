"""The planner's part of DSP_OP_REFLECTED_CONVOLVE on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/reflect_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the op with wild lengths, tap counts, slots, bindings, offsets
and strides, alone and with an avg_current behind it: each is planned -- on dsp_reflect_kernel, with an argument block whose bindings have
the right kind and size and which fits the kernel's LDS -- or refused with a reason."""
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
    exe = str(tmp_path_factory.mktemp("reflect_plan_fuzz") / "reflect_plan_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "reflect_plan_fuzz.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    return exe


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("DSPEED_HIP_"):
            del env[k]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [0x19F, 4])
def test_programs_with_the_op_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = _run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # both shapes (the fused one with the filtered row stored and not) and both geometries were planned ...
    assert rep["plain"] > 1000 and rep["fused"] > 800 and 300 < rep["fused_row_stored"] < rep["fused"] - 300, rep
    assert rep["accepted"] == rep["plain"] + rep["fused"] == rep["narrow"] + rep["wide"] and rep["narrow"] > 300 and rep["wide"] > 1000, rep
    # ... and the refusals by name were reached: the shapes', the kernel longer than the rows, the limits'
    assert rep["refused_shape"] > 300 and rep["refused_long"] > 500 and rep["refused_limit"] > 500 and rep["refused_by_name"] > 3000, rep
