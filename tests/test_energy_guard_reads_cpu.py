"""Where the register-resident energy kernel's lanes read their lagged streams, on the CPU: dsp_energy_rr::lag_window_start and
dsp_energy_rr::layout of dspeed_amd/csrc/dsp_kernels.h, the functions the kernel itself calls, in a stand-alone program
(tests/energy_guard_reads_check.cpp).  For C = 18, 34, 66, 130 samples a lane, every lane and every lag from 1 to 64 C + 200:

  * a window wholly below sample 0 reads inside the guard with every pair it can touch, at an even address that equals its natural one
    modulo 64 elements; every other window keeps its natural start and stays inside guard, image and tail;
  * the 32 lanes of either half of the wavefront read 32 different bank pairs;
  * layout(C) keeps its invariants (guard >= 2 C + 8 and >= C + 72, slot_off >= guard and a multiple of 4, an odd side pitch that holds
    the group sums), and the region of the wavefronts a compute unit runs (8; 4 at 8192 samples, which never had room for more) stays
    within 160 KB."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspeed_amd", "csrc")


def test_guard_reads_and_layout_by_brute_force(tmp_path):
    # any host C++17 compiler: g++, the system's c++ / clang++, or the clang++ of the ROCm that builds the library
    from dspeed_amd.build import _llvm_tool

    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or _llvm_tool("clang++")
    assert cxx, "no host C++ compiler (g++, c++, clang++, ROCm's clang++): the kernel's address rule cannot be checked"
    exe = str(tmp_path / "energy_guard_reads_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "energy_guard_reads_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    # 4 chunk lengths x 64 lanes x the lags; most lags leave some lane's window below sample 0, and most of those are not where they were
    assert rep["windows"] == 64 * sum(64 * c + 200 for c in (18, 34, 66, 130))
    assert rep["redirected"] > rep["windows"] // 4 and rep["moved"] > rep["redirected"] // 2
