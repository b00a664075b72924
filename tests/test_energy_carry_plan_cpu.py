"""The carry plan of the register-resident energy kernel (EnergyPlan, built by dsp_internal_plan_energy_carries in dsp_plan.cpp) on the CPU:
against a restatement in Python through the product library, and as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/energy_carry_plan_check.cpp, in the manner of tests/test_planner_fuzz.py)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import energy_carry_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspeed_amd", "csrc")


class EnergyPlan(C.Structure):
    _fields_ = [(name, (C.c_int32 * 4) * 3) for name in ("shift", "cs", "local", "grp", "side", "pn")]


def _plan(chunk, S, lags):
    from dspeed_amd import _lib

    fn = _lib.lib().dsp_internal_plan_energy_carries
    fn.argtypes, fn.restype = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(EnergyPlan)], None
    plan = EnergyPlan()
    fn(chunk, S, (C.c_int32 * 3)(*lags), C.byref(plan))
    return plan


def _hold(wf_len, S, lags):
    chunk = K.chunk(wf_len)
    plan = _plan(chunk, S, lags)
    for k, lag in enumerate(lags):
        for s in range(S):
            r, shift = K.capture_point(chunk, S, s, lag)
            # by brute force: the sample the lagged window of sub-chain s of lane j starts at is sample r of lane j - shift
            j = 40
            assert (j - shift) * chunk + r == j * chunk + s * ((chunk - 2) // S) - lag and 0 <= r < chunk
            got = (plan.grp[k][s], plan.side[k][s], plan.pn[k][s])
            assert plan.shift[k][s] == shift and got == K.split(r), (wf_len, S, lag, s, r, got, K.split(r))
            grp, side, pn = got
            assert plan.cs[k][s] * ((chunk - 2) // S) + plan.local[k][s] == r
            assert grp + pn == r and 0 <= pn <= 8 and (pn > 0 or r == 0) and side == grp // 8 - 1 and grp % 8 == 0
            assert grp <= chunk - 2 and side <= (chunk - 2) // 8 - 1  # the pairs start inside the chunk, the side array has the element


def test_split_is_the_prefix_position_counted_off_sample_by_sample():
    for r in range(0, 131):
        before = list(range(r))  # samples in front of the capture point
        groups = [before[i:i + 8] for i in range(0, len(before), 8)]
        want = (8 * (len(groups) - 1), len(groups) - 2, len(groups[-1])) if groups else (0, -1, 0)
        assert K.split(r) == want, r


@pytest.mark.parametrize("wf_len", K.LENGTHS)
def test_edge_capture_points(wf_len):
    chunk = K.chunk(wf_len)
    for S in (1, 2):
        for edge in K.edge_points(chunk):
            for shift in range(4):
                lag = shift * chunk + (chunk - edge) % chunk
                if lag > 0:
                    _hold(wf_len, S, (lag, lag + 1, 2 * lag + 1))
    for g in K.carry_geometries(wf_len):
        _hold(wf_len, 1, K.lags_of("trap_filter", g))


def test_random_geometries():
    rng = np.random.default_rng(6)
    for _ in range(3000):
        wf_len = int(rng.choice(K.LENGTHS))
        rise = int(rng.integers(1, wf_len // 2))
        flat = int(rng.integers(0, wf_len - 2 * rise + 1))
        fall = int(rng.integers(1, wf_len - rise - flat + 1))
        _hold(wf_len, int(rng.integers(1, 3)), (rise, rise + flat, 2 * rise + flat if rng.integers(2) else rise + flat + fall))


def test_the_plan_builder_runs_clean_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")
    exe = str(tmp_path / "energy_carry_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "energy_carry_plan_check.cpp"),
                           os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "5000", "11"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["sets"] == 5000 and rep["entries"] > 20000
