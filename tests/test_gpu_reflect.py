"""reflected_convolve_wf on the device (dsp_reflect.hip): the whole book of tests/reflect_cases.py against its emulation -- every bit in the
float32 loop, the project's 1e-12 FIR bar in the float64 loop and every bit on its integer class --, through the gufunc and, for the
layouts a gufunc call cannot make (padded strides, element offsets 0 .. 3 on both sides, a sentinel behind every output row), through the C
entry; the integer class against the reference's own float32 results; the shared loader's boundary samples; the fused avg_current against
the two gufuncs apart; the SiPM recipe fragment behind the filter, bit for bit against the CPU models; the refusals."""
import os

import numpy as np
import pytest

import extrema_cases as ec
import histogram_cases as hc
import reflect_cases as rc

pytestmark = pytest.mark.gpu

M = "dspeed.processors"
SENTINEL = -7.0
CODES = {"f32": "F32", "i16": "I16", "u16": "U16", "f64": "F64"}


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(want))


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    r, c = np.nonzero(bad)
    return len(r), sorted(set(r.tolist()))[:6], c[:6].tolist(), got[bad][:4], want[bad][:4]


def _holds(rows, n, m, name, got, want):
    """float32 loop: every bit.  float64 loop: 1e-12 of the row's largest reference value, the same non-finite pattern,
    and every bit on the integer class"""
    if rows != "f64" or rc.integer_class(rows, n, m, name):
        fin = [r for r in rc.finite_rows(rows) if r < len(want)] if rows == "f64" else range(len(want))
        return _same(np.ascontiguousarray(got[list(fin)]), np.ascontiguousarray(want[list(fin)])) and _holds_f64(got, want)
    return _holds_f64(got, want)


def _holds_f64(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    for g, w in zip(got, want):
        fin = np.isfinite(w)
        if not (np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)])):
            return False
        if fin.any() and not (np.abs(g[fin] - w[fin]) <= 1e-12 * np.abs(w[fin]).max()).all():
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------- 1. the whole book
@pytest.mark.parametrize("rows", list(rc.ROWS))
def test_the_whole_book_through_the_gufunc(rows):
    from dspeed_amd.processors import reflected_convolve_wf

    loop = rc.LOOPS[rows]
    seen = set()
    for index, n, m, name, k in rc.cases(rows):
        w = rc.rows_of(rows, n)
        want = rc.want(rows, n, m, name, index)
        out = np.full((len(w), n), SENTINEL, dtype=loop)
        assert reflected_convolve_wf(w, k, out) is out
        assert _holds(rows, n, m, name, out, want), (rows, n, m, name, _diff(out, want))
        seen.add(name)
        if name == "nan":
            assert np.isnan(out).all()
        if name == "zero" and rows in ("f32", "f64") and m >= 2:  # the +inf row under a kernel with a zero tap: inf x 0 where the window covers it
            row = out[rc.families(rows).index("inf")]
            assert np.isnan(row).any() and np.isnan(row).sum() == np.isnan(want[rc.families(rows).index("inf")]).sum()
    assert seen == {"asym", "gauss", "zero", "nan"}
    got = reflected_convolve_wf(rc.rows_of(rows, 64), rc.asymmetric(9).astype(loop))  # the output left out: a new array of the loop's type
    assert _holds(rows, 64, 9, "asym", got, rc.emulate(rc.rows_of(rows, 64), rc.asymmetric(9), loop))
    one = reflected_convolve_wf(rc.rows_of(rows, 64)[0], rc.asymmetric(9).astype(loop))  # a 1-D call
    assert one.shape == (64,) and _holds(rows, 64, 9, "asym", one[None], rc.emulate(rc.rows_of(rows, 64)[:1], rc.asymmetric(9), loop))


@pytest.mark.parametrize("rows", list(rc.ROWS))
def test_layouts_through_the_c_entry_with_sentinels(rows):
    """rows n + 0 .. 3 apart from an element 0 .. 3 past a 16-byte boundary on the way in, likewise on the way out: 16-byte loads and stores
    where start and stride allow, a sample per lane otherwise, and nothing but the n samples of every row written; row counts 1, 3, 4, 5
    and 130"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.gufunc import run

    fn = _lib.lib().dsp_reflected_convolve_rows
    loop = rc.LOOPS[rows]
    esz, isz = np.dtype(loop).itemsize, np.dtype(rc.ROWS[rows]).itemsize
    loop_code, code = _lib.F32 if loop is np.float32 else _lib.F64, getattr(_lib, CODES[rows])
    vectors = set()
    for index, n, m, name, k in rc.cases(rows):
        if name != "asym":
            continue
        base, base_want = rc.rows_of(rows, n), rc.want(rows, n, m, name, index)
        R = rc.ROW_COUNTS[index % len(rc.ROW_COUNTS)] if n <= 300 else rc.ROW_COUNTS[index % 4]
        reps = -(-R // len(base))
        w, want = np.tile(base, (reps, 1))[:R], np.tile(base_want, (reps, 1))[:R]
        in_off, in_stride = index % 4, n + (index // 4) % 4
        off, out_stride = (index // 2) % 4, n + (index // 3) % 3
        block = np.full(8 + R * in_stride, 77, dtype=w.dtype)
        block[in_off:in_off + R * in_stride].reshape(R, in_stride)[:, :n] = w
        blank = np.full(4 + R * out_stride + 8, SENTINEL, dtype=loop)
        d, o, kd = DeviceArray.from_numpy(block), DeviceArray.from_numpy(blank), DeviceArray.from_numpy(np.ascontiguousarray(k, dtype=loop))
        assert o.ptr % 16 == 0 and d.ptr % 16 == 0
        vectors.add((in_off * isz % 16 == 0 and in_stride * isz % 16 == 0 and n * isz % 16 == 0, off == 0 and out_stride * esz % 16 == 0))
        run(fn, "reflected_convolve_wf", d.ptr + in_off * isz, code, R, n, in_stride, loop_code, kd.ptr, m, o.ptr + off * esz, out_stride)
        got = o.to_numpy()
        body = got[off:off + R * out_stride].reshape(R, out_stride)
        assert _holds(rows, n, m, name, np.ascontiguousarray(body[:, :n])[:len(base)], want[:len(base)]), (rows, n, m, _diff(body[:, :n], want))
        assert _holds_f64(np.ascontiguousarray(body[:, :n]), want), (rows, n, m, R)
        assert (got[:off] == SENTINEL).all() and (body[:, n:] == SENTINEL).all() and (got[off + R * out_stride:] == SENTINEL).all(), (rows, n, m)
        assert d.to_numpy().tobytes() == block.tobytes()  # (the rows are read, never written)
        d.free(), o.free(), kd.free()
    assert {v[0] for v in vectors} == {True, False} and {v[1] for v in vectors} == {True, False}


# ---------------------------------------------------------------------------------------------------------------- 2. the reference's float32
def test_the_integer_class_against_the_reference_float32_fixture():
    from dspeed_amd.processors import reflected_convolve_wf

    book = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{rc.BOOK}.npz"))
    checked = 0
    for key, n, m, name, k in rc.fixture_cases("f32"):
        if not rc.integer_class("f32", n, m, name):
            continue
        ref = book[f"{key}/f32"]
        fin = rc.finite_rows("f32")
        got = reflected_convolve_wf(rc.rows_of("f32", n), k)
        assert np.array_equal(got[fin], ref[fin]), (key, _diff(got[fin], ref[fin]))
        checked += 1
    assert checked > 50


# ---------------------------------------------------------------------------------------------------------------- 3. the loader's boundaries
@pytest.mark.parametrize("rows", list(rc.ROWS))
def test_the_shared_loaders_boundary_samples(rows):
    """A spike on N - 1, N, 64 N - 1, 64 N, 64 N K - 1, 64 N K and n - 1 (N samples of 16 bytes, K groups in flight), read 16 bytes a lane
    (whole-vector rows) and a sample a lane (the rows one element off): the rule of tests/test_gpu_row_stream.py, for this kernel"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.gufunc import run

    fn = _lib.lib().dsp_reflected_convolve_rows
    loop, dt = rc.LOOPS[rows], rc.ROWS[rows]
    esz, isz = np.dtype(loop).itemsize, np.dtype(dt).itemsize
    loop_code, code = _lib.F32 if loop is np.float32 else _lib.F64, getattr(_lib, CODES[rows])
    N = 16 // isz
    k = rc.asymmetric(3).astype(loop)
    kd = DeviceArray.from_numpy(k)
    for n in (64 * N * 4 + 64 * N, 64 * N * 8 + 16 * N):  # (K = 4 with vectors, 8 without: both kinds of group past one turn of the loop)
        for K in (4, 8):
            spikes = sorted({p for p in (N - 1, N, 64 * N - 1, 64 * N, 64 * N * K - 1, 64 * N * K, n - 1) if p < n})
            w = np.full((len(spikes), n), 2, dtype=dt)
            for r, p in enumerate(spikes):
                w[r, p] = 1000
            want = rc.emulate(w, k, loop)
            for shift in (0, 1):  # 16-byte loads; the same rows one element off: a sample per lane
                block = np.full(len(spikes) * n + 16, 55, dtype=dt)
                block[shift:shift + w.size] = w.reshape(-1)
                d, o = DeviceArray.from_numpy(block), DeviceArray((len(spikes), n), loop)
                run(fn, "reflected_convolve_wf", d.ptr + shift * isz, code, len(spikes), n, n, loop_code, kd.ptr, 3, o.ptr, n)
                got = o.to_numpy()
                assert _same(got, want), (rows, n, K, shift, _diff(got, want))
                d.free(), o.free()
    kd.free()


# ---------------------------------------------------------------------------------------------------------------- 4. fused against apart
@pytest.mark.parametrize("n, m", [(1000, 9), (64, 64), (rc.T - 8, 9), (rc.T - 7, 9), (4096, 65)])
def test_the_fused_current_equals_the_two_gufuncs_apart(n, m):
    """curr of LOAD, REFLECTED_CONVOLVE, AVG_CURRENT, STORE [, STORE], in every bit, is avg_current of reflected_convolve_wf's output;
    lengths 5 and 1, the filtered row stored and not, both geometries; a row with a NaN, and one whose filtered row holds NaNs (a +inf
    under a zero tap): NaN currents, as the two launches give"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray, sync
    from dspeed_amd.processors import avg_current, reflected_convolve_wf

    w = rc.rows_of("f32", n)
    for name, k in (("asym", rc.asymmetric(m).astype(np.float32)), ("zero", rc.kernels_of(n, m, np.float32, 1).get("zero"))):
        g = reflected_convolve_wf(w, k)
        assert _same(g, rc.emulate(w, k, np.float32))
        for lag in (5, 1):
            apart = avg_current(g, lag, np.empty((len(w), n - lag), np.float32))
            assert _same(apart, rc.avg_current(g, lag)), (n, m, name, lag)
            for store_row in (True, False):
                chain = Chain(rc.program(n, m, lag=lag, store_row=store_row), compute_dtype=np.float32)
                assert chain.kernel_name == rc.KERNEL
                assert chain.geometry(len(w))["blocks"] == (len(w) if rc.wide(n, m, "f32") else -(-len(w) // 4))
                dev = {"w": DeviceArray.from_numpy(w), "taps:k": DeviceArray.from_numpy(k),
                       "curr": DeviceArray.from_numpy(np.full((len(w), n - lag), SENTINEL, np.float32))}
                if store_row:
                    dev["out"] = DeviceArray.from_numpy(np.full((len(w), n), SENTINEL, np.float32))
                chain.execute(dev, len(w))
                sync()
                chain.check()
                curr = dev["curr"].to_numpy()
                assert _same(curr, apart), (n, m, name, lag, store_row, _diff(curr, apart))
                assert not store_row or _same(dev["out"].to_numpy(), g)
                chain.close()
                for d in dev.values():
                    d.free()


# ---------------------------------------------------------------------------------------------------------------- 5. the recipe
def _recipe():
    procs = {"wf_gaus": {"function": "reflected_convolve_wf", "module": f"{M}.convolutions", "args": ["waveform", "db.kernel", "wf_gaus"], "unit": "ADC"}}
    procs.update(hc.sipm_fragment("wf_gaus"))
    return procs


def test_the_sipm_fragment_behind_the_filter_bit_for_bit():
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain
    from dspeed_amd.processors import gaussian_filter1d

    w = hc.sipm_rows()
    k = gaussian_filter1d(np.float32(1), np.float32(4), np.empty(9, np.float32))
    outputs = ["wf_gaus", "curr", "fwhm", "idx_out_c", "max_out", "vt_max_candidate_out", "vt_min_out", "n_max_out", "n_min_out"]
    chain, _, out = build_processing_chain({"outputs": outputs, "processors": _recipe()}, {"waveform": WaveformInput(w, 16.0)},
                                           db_dict={"kernel": k})
    chain.execute()
    kernels = [kern for _w, kern in chain.kernels()]
    assert kernels.count(rc.KERNEL) == 1 and "dsp_hist_kernel" in kernels and "dsp_extrema_kernel" in kernels
    g = rc.emulate(w, k, np.float32)
    assert _same(out["wf_gaus"], g), _diff(out["wf_gaus"], g)
    assert _same(out["curr"], rc.avg_current(g, 5)), _diff(out["curr"], rc.avg_current(g, 5))
    # everything downstream against the CPU models of the two kernels, run on the device's own current (each model is held against the
    # reference's bodies by its own CPU test)
    names = ["vt_max_candidate_out", "vt_min_out", "n_max_out", "n_min_out", "fwhm", "idx_out_c", "max_out"]
    want = {key: [] for key in names}
    for row in np.asarray(out["curr"]):
        wts, brd = hc.model_histogram(row, 100, np.float32, 1)
        mode, edge, fwhm = hc.model_stats(wts, brd, np.nan, np.float32)
        lists = ec.model(row, 5, 0.1, 1, np.float32(3) * fwhm, 0, 20, np.float32, 1)
        for key, v in zip(names, (*lists, fwhm, mode, edge)):
            want[key].append(v)
    for key in names:
        expect = np.array(want[key], dtype=np.uint32 if key.startswith("n_") else np.float32)
        got = np.asarray(out[key])
        assert got.dtype == expect.dtype and got.shape == expect.shape and np.array_equal(got, expect, equal_nan=True), key
    counts = np.array(want["n_max_out"])
    assert (counts == 0).any() and (counts > 1).any() and np.isfinite(np.array(want["fwhm"])).all()  # the rows are not trivial


# ---------------------------------------------------------------------------------------------------------------- 6. the refusals
def test_the_refusals_reached_from_the_gufunc():
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import reflected_convolve_wf as rcw

    with pytest.raises(DSPFatal, match="The filter is longer than the input waveform"):
        rcw(np.zeros((3, 8), np.float32), np.ones(9, np.float32))
    with pytest.raises(DSPFatal, match="The filter is longer than the input waveform"):
        rcw(np.full((3, 8), np.nan, np.float32), np.ones(9, np.float32))  # (for the whole call, even where every row holds a NaN)
    for rows in ("f32", "f64"):
        for n, m in rc.over_the_limit(rows):
            with pytest.raises(NotImplementedError, match=f"reflected_convolve_wf: {rc.LIMITS} \\(len\\(w_in\\) = {n}, len\\(kernel\\) = {m} given\\)"):
                rcw(np.zeros((1, n), rc.ROWS[rows]), np.ones(m, rc.LOOPS[rows]))
    with pytest.raises(ValueError, match="the output has the length of the input \\(len\\(w_in\\) = 8, len\\(w_out\\) = 9\\)"):
        rcw(np.zeros((3, 8), np.float32), np.ones(3, np.float32), np.zeros((3, 9), np.float32))
    with pytest.raises(NotImplementedError, match="the float64 loop takes float64 rows on the device"):
        rcw(np.zeros((3, 8), np.int32), np.ones(3, np.float64))
