"""What the CPU tests around the stand-alone C++ programs of this directory share: the compile line -- plain g++ with AddressSanitizer and
UndefinedBehaviorSanitizer, no HIP, no LD_PRELOAD --, the skip where g++ or its sanitizer runtime is missing, and the run that reads a
program's one-line JSON report."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspeed_amd", "csrc")
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include")]


def need_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")


def build(out_dir, name, with_planner=True):
    """tests/<name>.cpp, with the planner (dsp_plan.cpp alone: it needs no HIP) where the program calls it; the executable"""
    need_sanitizers()
    exe = str(out_dir / name)
    sources = [os.path.join(ROOT, "tests", name + ".cpp")] + ([os.path.join(CSRC, "dsp_plan.cpp")] if with_planner else [])
    subprocess.check_call(FLAGS + sources + ["-o", exe])
    return exe


def run(cmd, timeout=600):
    """the report a program prints last; the library's switches are taken out of its environment (the planner reads them: the default plan is what is fuzzed)"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("DSPEED_HIP_"):
            del env[k]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-6000:])
    return json.loads(r.stdout.strip().splitlines()[-1])
