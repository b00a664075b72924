"""The schedule of dsp_sort.hip and the planner's part of DSP_OP_SORT on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: two
stand-alone programs with a ``main`` of their own, plain g++, no HIP, no LD_PRELOAD.

``tests/sort_network.cpp`` includes ``dsp_kernels.h`` and runs the ``dsp_sort`` namespace -- the key map, the padding, every step's partner,
direction and kind -- for every length from 1 to 300 and every edge length of the case book, over the key map of the families: the result
must equal ``std::sort`` of the keys, in the schedule's order and in the order the kernel's passes run the steps; every step is exactly one
of register, cross-lane or LDS; no partner leaves [0, P).

``tests/sort_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the op with wild lengths, slots, offsets and strides: each is
planned -- on dsp_sort_kernel, with an argument block that fits its LDS -- or refused with a reason."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspeed_amd", "csrc")
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("DSPEED_HIP_"):
            del env[k]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_network_sorts_every_length_and_family(sanitizers, tmp_path):
    exe = str(tmp_path / "sort_network")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "sort_network.cpp"), "-o", exe])
    rep = _run([exe])
    # 12 padded lengths from 8 to 16384: 6 + 10 + .. + 105 steps; (300 + 16 lengths) x 9 families in float32, those up to 8192 in float64
    assert rep == {"steps": sum(k * (k + 1) // 2 for k in range(3, 15)), "rows": (316 + 314) * 9, "failures": 0}


@pytest.fixture(scope="module")
def fuzzer(sanitizers, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sort_plan_fuzz") / "sort_plan_fuzz")
    subprocess.check_call(FLAGS + [os.path.join(ROOT, "tests", "sort_plan_fuzz.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [0x50F7, 2])
def test_programs_with_the_op_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = _run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # both geometries were planned, and refusals by name were reached: the shape's and the limit's
    assert rep["narrow"] > 1000 and rep["wide"] > 1000 and rep["accepted"] == rep["narrow"] + rep["wide"] and rep["refused_by_name"] > 500, rep
