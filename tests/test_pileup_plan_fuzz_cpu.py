"""The planner's part of DSP_OP_RC_CR2 and DSP_OP_BI_LEVEL_ZERO_CROSSING on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: a
stand-alone program with a ``main`` of its own, plain g++, no HIP, nothing preloaded.

``tests/pileup_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the ops with wild lengths, list lengths, slots, bindings, offsets,
strides and operands -- the filter alone, the walk alone, both in one launch, each with or without a BL_SUBTRACT behind the LOAD --: each is
planned -- on dsp_pileup_kernel, with an argument block whose bindings have the right kind, type and size -- or refused with a reason."""
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
    exe = str(tmp_path_factory.mktemp("pileup_plan_fuzz") / "pileup_plan_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "pileup_plan_fuzz.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
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
    # every shape was planned: the filter, the walk, both in one launch with the filtered row stored and not, with a subtraction, with columns ...
    assert rep["filter"] > 500 and rep["walk"] > 300 and rep["fused"] > 300 and 100 < rep["fused_row_stored"] < rep["fused"] - 100, rep
    assert rep["accepted"] == rep["filter"] + rep["walk"] + rep["fused"] and rep["subtracted"] > 200 and rep["columns"] > 300, rep
    # ... and the refusals by name were reached: the shapes', the short rows', t_start's, the lists'
    assert rep["refused_shape"] > 300 and rep["refused_short"] > 20 and rep["refused_start"] > 100 and rep["refused_lists"] > 300 and rep["refused_by_name"] > 2000, rep
