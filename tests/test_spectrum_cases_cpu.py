"""psd and fft without a GPU: the NumPy model of dsp_spectrum.hip's formulation (tests/spectrum_cases.py) held to the rules the device is
held to -- exact bins, the error cap against NumPy's float64 rfft, psd against the model's own fft, the bar against the reference's float32
error, NaN rows as the reference writes them (tests/golden/spectrum.npz) --, the tables' exact entries, and the host's table code
(dsp_spectrum_tables.h) against the model's under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_util
import spectrum_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def book():
    return {c.name: c for c in golden_util.cases(sc.BOOK, kernel=sc.KERNEL)}


@pytest.fixture(scope="module")
def groups():
    return sc.groups()


def test_the_book_covers_what_it_has_to(book, groups):
    assert [g.name for g in groups] == list(book)
    f32 = {g.n for g in groups if g.rows == "f32"}
    f64 = {g.n for g in groups if g.rows == "f64"}
    assert set(sc.BASE) <= f32 and {2048, 4096, 511, 513, 4095} <= f32  # the base set, both sides of both switches, the longest other length
    assert f64 == {n for n in sc.LENGTHS if sc.admitted(n, np.float64)} and {1024, 2048, 255, 257, 2047, 8192} <= f64 and 16384 not in f64
    assert not sc.wide(2048, np.float32) and sc.wide(4096, np.float32) and not sc.wide(511, np.float32) and sc.wide(513, np.float32)
    assert not sc.wide(1024, np.float64) and sc.wide(2048, np.float64) and not sc.wide(255, np.float64) and sc.wide(257, np.float64)
    assert {g.rows for g in groups} == {"f32", "f64", "i16", "u16"}
    for g in groups:
        assert 2 <= len(g.w) <= 4 or g.n <= sc.LONG
        c = book[g.name]
        assert c.params["rows"] == g.names and c.params["stored"] == g.stored
        if g.stored:
            assert c["fft"].shape == (len(g.stored), g.n // 2 + 1) and c["fft"].dtype == (np.complex64 if g.tag == "f32" else np.complex128)
    assert os.path.getsize(os.path.join(golden_util.GOLDEN_DIR, sc.BOOK + ".npz")) < 512 * 1024


def test_the_reference_stays_within_the_cap_and_writes_nan_rows_as_documented(book, groups):
    """what the rules take from the reference: its float32 error is inside the cap on every finite row, a NaN row is NaN + 0j in every bin --
    and a row with an infinity is the mix of NaN and inf that the device does not copy"""
    mixed = 0
    for g in groups:
        c, X64 = book[g.name], g.truth()
        for k, r in enumerate(g.stored):
            ref = c["fft"][k]
            if g.names[r].startswith("nan_"):
                sc.check_nan(ref, True)
                if "psd" in c:
                    sc.check_nan(c["psd"][k], False)
            elif g.names[r] == "inf_mid":
                mixed += int(np.isinf(ref.real).any() or np.isinf(ref.imag).any() or (ref.imag != 0).any())
            else:
                assert sc.rel_l2(ref, X64[r]) <= sc.cap(g.n, g.loop), (g.name, g.names[r])
    assert mixed >= 10


def test_the_model_of_the_kernel_keeps_every_rule(book, groups):
    ratios = {}
    for g in groups:
        X = np.stack([sc.model_fft(w, g.loop) for w in g.w])
        P = np.stack([sc.model_psd(w, g.loop) for w in g.w])
        figures = sc.check_group(g, book[g.name], X, P, "model")
        if figures.get("noise", (0, None))[1] is not None:
            ratios[g.name] = figures["noise"][1]
    # the bars hold with room: plain radix 2 within 6 of the reference's error, Bluestein within 9
    assert len(ratios) >= 25 and max(v for k, v in ratios.items() if sc.pow2(int(k.split("_n")[1]))) < 6 and max(ratios.values()) < 9, ratios


def test_the_rules_tell_a_wrong_spectrum(book, groups):
    """a twiddle of the last pass rounded once more, a conjugated bin, a bin that is not NaN: each is caught"""
    g = next(g for g in groups if g.name == "f32_n1024")
    X = np.stack([sc.model_fft(w, g.loop) for w in g.w])
    P = np.stack([sc.model_psd(w, g.loop) for w in g.w])
    sc.check_group(g, book[g.name], X, P)
    for r, k, value in ((0, 5, None), (3, 7, 1e-3 + 0j), (6, 0, 0j), (1, 3, "scale")):
        bad = X.copy()
        bad[r, k] = np.conj(X[r, k]) if value is None else (X[r, k] * np.complex64(1 + 1e-4) if value == "scale" else value)
        with pytest.raises(AssertionError):
            sc.check_group(g, book[g.name], bad, P)
    bad = P.copy()
    bad[0, 9] *= np.float32(1 + 1e-6)
    with pytest.raises(AssertionError):
        sc.check_group(g, book[g.name], X, bad)


def test_the_tables_hold_the_exact_entries():
    for T in (np.float32, np.float64):
        for n in (2, 4, 8, 64, 1024, 16384 if T is np.float32 else 8192):
            tw, aux, filt = sc.tables(n, T)
            L = sc.points(n)
            assert filt is None and len(aux[0]) == n // 2 + 1 and len(tw[0]) == L // 2
            assert (aux[0][0], aux[1][0]) == (1, 0) and (aux[0][n // 2], aux[1][n // 2]) == (-1, 0)
            if n >= 4:
                assert (aux[0][n // 4], aux[1][n // 4]) == (0, -1)
            if L >= 4:
                assert (tw[0][0], tw[1][0]) == (1, 0) and (tw[0][L // 4], tw[1][L // 4]) == (0, -1)
        for n in (3, 20, 1000, 4095 if T is np.float32 else 2047):
            tw, chirp, filt = sc.tables(n, T)
            L = sc.points(n)
            assert L >= 2 * n - 1 and L < 2 * (2 * n - 1) and len(chirp[0]) == n and len(filt[0]) == L
            assert (chirp[0][0], chirp[1][0]) == (1, 0)
            # j^2 modulo 2 n in integers: j = n / 2 of n = 20 is the angle -pi * 100 / 20 = -5 pi, exactly -1; of n = 1000 an even number of turns, 1
            if n == 20:
                assert (chirp[0][10], chirp[1][10]) == (-1, 0)
            if n == 1000:
                assert (chirp[0][500], chirp[1][500]) == (1, 0)
            mag = np.hypot(chirp[0].astype(np.float64), chirp[1].astype(np.float64))
            assert np.abs(mag - 1).max() <= 2 * sc.eps(T)


PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "dsp_spectrum_tables.h"
#include "dsp_kernels.h"
int main(int argc, char** argv) {
    namespace tb = dsp_spectrum_tables;
    for (int a = 1; a < argc; ++a) {
        const int n = atoi(argv[a]), L = dsp_spectrum::points(n);
        int bits = 0;
        while ((1 << bits) < L) ++bits;
        printf("n %d points %d wide32 %d wide64 %d lds32 %d lds64 %d\n", n, L, (int)dsp_spectrum::wide(n, 4), (int)dsp_spectrum::wide(n, 8),
               dsp_spectrum::lds_bytes(n, 4), dsp_spectrum::lds_bytes(n, 8));
        const bool p2 = dsp_spectrum::pow2(n);
        std::vector<std::vector<double>> t = {tb::twiddle(L), p2 ? tb::unpack(n) : tb::chirp(n)};
        if (!p2) t.push_back(tb::filter(n, L, bits));
        for (const auto& v : t) {
            printf("table %zu\n", v.size() / 2);
            for (double x : v) printf("%.17g\n", x);
        }
    }
    return 0;
}
"""


def test_the_host_s_tables_are_the_model_s(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("g++ has no AddressSanitizer runtime here")
    src, exe = tmp_path / "spectrum_tables.cpp", tmp_path / "spectrum_tables"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "dspeed_amd", "csrc"),
                           str(src), "-o", str(exe)])
    lengths = [1, 2, 3, 4, 5, 8, 20, 64, 65, 511, 513, 1000, 1024, 2048, 4095, 4096]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)] + [str(n) for n in lengths], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.split("\n"))
    for n in lengths:
        head = next(lines).split()
        L = sc.points(n)
        assert head[:4] == ["n", str(n), "points", str(L)], head
        assert (int(head[5]), int(head[7])) == (int(sc.wide(n, np.float32)), int(sc.wide(n, np.float64)))
        for esz, at in ((4, 9), (8, 11)):
            assert int(head[at]) == (L * 2 * esz + 16 if L * 2 * esz > sc.WAVE_ROW_BYTES else 4 * L * 2 * esz)
        for t in sc.tables(n, np.float64):
            if t is None:
                continue
            count = int(next(lines).split()[1])
            assert count == len(t[0]), (n, count, len(t[0]))
            if not count:
                continue
            got = np.array([float(next(lines)) for _ in range(2 * count)]).reshape(count, 2)
            # (libm beside NumPy: an ulp of a value of magnitude 1; the filter's bins are sums of n such values, divided by the points)
            scale = max(1.0, np.hypot(t[0], t[1]).max())
            assert np.abs(got[:, 0] - t[0]).max() <= 1e-13 * scale and np.abs(got[:, 1] - t[1]).max() <= 1e-13 * scale, n
            exact = (np.hypot(t[0], t[1]) == 1) & ((t[0] == 0) | (t[1] == 0)) if len(t[0]) != L or sc.pow2(n) else np.zeros(count, bool)
            assert np.array_equal(got[exact, 0], t[0][exact]) and np.array_equal(got[exact, 1], t[1][exact])
