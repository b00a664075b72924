"""The single-processor entry points (``dspeed_amd/csrc/dsp_gufuncs.cpp``) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer.

Every ``dsp_<name>_f32`` / ``_f64`` is a tiny cached chain: the entry point builds a ``dsp_op`` program, looks it up in a cache, and hands it to
``dsp_chain_create`` / ``execute`` / ``check``.  ``tests/gufunc_programs.cpp`` calls each of them against stand-ins for those functions and
prints the program, the io descriptors, the order of the io pointers and the return code of every call; this test compares that text with
``tests/golden/gufunc_programs.txt.gz``, EXACTLY (gzip: 90 kB of recording are nothing to read in a diff; ``zcat`` shows them).  The fixture
was recorded (``tools/record_gufunc_programs.py``) from the entry points as they stood in ``dsp_host.cpp``, moved into their own file and otherwise untouched: a slip in the order of ``add_slot`` / ``add_io`` / ``add_op``, in
an ``ip[]`` or in which argument becomes which io pointer shows here, not as a wrong number on the device."""
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dspeed_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gufunc_programs.txt.gz")


def build_program(exe):
    """the entry points, the planner (for dsp_fail / dsp_fatal_message) and the test program: plain g++, no HIP, no LD_PRELOAD"""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "gufunc_programs.cpp"),
                           os.path.join(CSRC, "dsp_gufuncs.cpp"), os.path.join(CSRC, "dsp_plan.cpp"), "-o", exe])
    return exe


def run_program(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-6000:])
    return r.stdout


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")
    return run_program(build_program(str(tmp_path_factory.mktemp("gufunc_programs") / "gufunc_programs")))


def _by_call(text):
    """{first line of a record: the record}; a record starts at a line that is not indented"""
    out, head = {}, None
    for line in text.splitlines():
        if not line.startswith(" "):
            head = line
            n = 2
            while head in out:  # (the same call made again: the cached chain)
                head = f"{line} ({n})"
                n += 1
            out[head] = []
        out[head].append(line)
    return out


def test_every_entry_point_builds_the_recorded_program(records):
    with gzip.open(GOLDEN, "rt") as f:
        golden = f.read()
    got, want = _by_call(records), _by_call(golden)
    assert list(got) == list(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, "\n".join(["records that differ from tests/golden/gufunc_programs.txt.gz:"] + [line for k in differ[:3] for line in ["-- recorded"] + want[k] + ["-- now"] + got[k]])
    assert records == golden


def test_the_program_calls_every_exported_entry_point(records):
    """(the header is the list: a processor added to it and not to tests/gufunc_programs.cpp fails here)"""
    import re

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dspeed_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+dsp_([a-z0-9_]+)_(f32|f64)\s*\(", text, flags=re.M))
    assert len(declared) >= 54  # (the scan sees them: 27 processors, two loops each)
    called = set(re.findall(r"^([a-z0-9_]+?)(?:/[^\n]*?)?_(f32|f64) n_wf=3$", records, flags=re.M))
    assert declared <= called, sorted(declared - called)


def test_the_entry_points_include_no_hip_header():
    src = open(os.path.join(CSRC, "dsp_gufuncs.cpp")).read()
    assert "#include <hip" not in src and "dsp_launch.h" not in src
