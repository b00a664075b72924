"""The planner's part of DSP_OP_PEAK_SNR_THRESHOLD and DSP_OP_MULTI_A_FILTER on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/pulse_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild lengths, list lengths, slots, bindings, offsets,
strides and operands -- the picker alone, the pick-off alone, both in one launch with the packed list stored or not --: each is planned -- on
dsp_pulses_kernel, with an argument block whose bindings have the right kind, type and size and whose list, width and lengths keep the
kernel's bounds -- or refused with a reason."""
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
    exe = str(tmp_path_factory.mktemp("pulse_plan_fuzz") / "pulse_plan_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "pulse_plan_fuzz.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    return exe


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("DSPEED_HIP_"):
            del env[k]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [0x31, 9])
def test_programs_with_the_ops_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = _run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # every shape was planned: the picker, the pick-off, both in one launch with the packed list stored and not, the ratio a column ...
    assert rep["picker"] > 500 and rep["pickoff"] > 500 and rep["fused"] > 500 and 100 < rep["fused_list_stored"] < rep["fused"] - 100, rep
    assert rep["accepted"] == rep["picker"] + rep["pickoff"] + rep["fused"] and rep["ratio_columns"] > 200, rep
    # ... and the refusals by name were reached: the shapes', the long lists', the width's, the outputs' lengths, the pick-off's return array
    assert rep["refused_shape"] > 300 and rep["refused_long"] > 100 and rep["refused_width"] > 100 and rep["refused_lengths"] > 300, rep
    assert rep["refused_return"] > 50 and rep["refused_by_name"] > 2000, rep
