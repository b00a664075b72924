"""peak_snr_threshold and multi_a_filter on the device (dsp_pulses.hip): the whole book of tests/pulse_cases.py against its emulation --
every bit, both loops, lists, counts and amplitudes -- through the gufuncs with NumPy and with DeviceArray arguments, through the C entries
for the layouts a gufunc call cannot make (an element offset, padded strides, int16 and uint16 rows, a canary around every output row),
through the fused launch against the two calls apart, and through a recipe; the fatal path; the SiPM fragment on synthetic rows."""
import numpy as np
import pytest

import pulse_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
CODES = {np.dtype(np.float32): "F32", np.dtype(np.int16): "I16", np.dtype(np.uint16): "U16", np.dtype(np.float64): "F64"}


def _same(got, want):
    return (got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
            and np.array_equal(np.signbit(got), np.signbit(want)))


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return int(bad.sum()), [i[:6].tolist() for i in np.nonzero(bad)], got[bad][:4], want[bad][:4]


@pytest.fixture(scope="module")
def emulated():
    """the emulation of the whole book, once: {key: (case, idx_out, count, amplitudes of idx_out or None, fatal rows or None)}; read only"""
    out = {}
    for loop, T in pc.LOOPS.items():
        for c in pc.all_cases(loop):
            idx, count, _trace = pc.emulate_picker(c["rows"], c["lists"], c["ratio"], c["width"], T)
            amp, fatal = pc.emulate_pickoff(c["rows"], idx, T) if c["m"] < c["n"] else (None, None)
            for a in (idx, count, amp, fatal):
                if a is not None:
                    a.setflags(write=False)
            out[c["key"]] = (c, idx, count, amp, fatal)
    return out


def _of_loop(emulated, loop):
    return [v for k, v in emulated.items() if f"_{loop}_" in k]


def _row_count(c, index):
    """rows of a launch: a block of named rows whole (at least), a sweep's rows over and over to one of ROW_COUNTS"""
    return max(pc.ROW_COUNTS[index % len(pc.ROW_COUNTS)], len(c["rows"]) if c["key"].startswith("named") else 0)


def _without_fatal(c, idx, count, amp, fatal):
    """the case without the rows whose kept candidates are fractional (the pick-off raises on them: test_..._names_its_row)"""
    keep = ~fatal
    c = dict(c, rows=c["rows"][keep], lists=c["lists"][keep], ratio=c["ratio"][keep], names=[nm for nm, k in zip(c["names"], keep) if k])
    return c, idx[keep], count[keep], amp[keep]


# ---------------------------------------------------------------------------------------------------------------- 1. the gufuncs
@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_book_through_the_gufuncs_with_numpy_arguments(emulated, loop):
    """outputs passed in and left out in turn; a ratio per row, and the constant where the case has one for all rows"""
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import multi_a_filter, peak_snr_threshold

    T = pc.LOOPS[loop]
    constants = fatal_calls = 0
    for index, (c, idx, count, amp, fatal) in enumerate(_of_loop(emulated, loop)):
        R = _row_count(c, index)
        w, lists, ratio = pc.tile_rows(c["rows"], R), pc.tile_rows(c["lists"], R), pc.tile_rows(c["ratio"], R)
        want_idx, want_n = pc.tile_rows(idx, R), pc.tile_rows(count, R)
        same_ratio = bool((ratio == ratio[0]).all())
        constants += int(same_ratio)
        if index % 2:
            oi, on = np.full((R, c["m"]), SENTINEL, T), np.full(R, 77, np.uint32)
            got = peak_snr_threshold(w, lists, T(ratio[0]) if same_ratio else ratio, c["width"], oi, on)
            assert got[0] is oi and got[1] is on
        else:
            oi, on = peak_snr_threshold(w, lists, ratio, float(c["width"]))
        assert on.dtype == np.uint32 and np.array_equal(on, want_n), (c["key"], R, [c["names"][k % len(c["names"])] for k in np.flatnonzero(on != want_n)][:6])
        assert _same(oi, want_idx), (c["key"], R, _diff(oi, want_idx))
        if amp is None:
            continue
        ok = ~pc.tile_rows(fatal, R)
        if ok.all():
            oa = np.full((R, c["m"]), SENTINEL, T) if index % 2 else None
            ga = multi_a_filter(w, oi, oa) if oa is not None else multi_a_filter(w, oi)
            assert (oa is None or ga is oa) and _same(ga, pc.tile_rows(amp, R)), (c["key"], R, _diff(ga, pc.tile_rows(amp, R)))
        else:  # a fractional candidate that is kept: the reference's DSPFatal, for the first such row; the others alone are right
            with pytest.raises(DSPFatal, match="^fixed_time_pickoff requires integer t_in when using mode 'i'\n") as e:
                multi_a_filter(w, oi)
            assert e.value.wf_range.start in np.flatnonzero(~ok)
            assert _same(multi_a_filter(w[ok], oi[ok]), pc.tile_rows(amp, R)[ok])
            fatal_calls += 1
        # the case's own list, NaNs where they stand
        direct, direct_fatal = pc.emulate_pickoff(c["rows"], c["lists"], T)
        keep = ~pc.tile_rows(direct_fatal, R)
        assert _same(multi_a_filter(w[keep], lists[keep]), pc.tile_rows(direct, R)[keep]), c["key"]
    assert constants > 20 and fatal_calls >= 1
    # 1-D calls
    c, idx, count, amp, _fatal = emulated[f"sweep_{loop}_n65_m20_w10"]
    oi, on = peak_snr_threshold(c["rows"][0], c["lists"][0], T(c["ratio"][0]), 10)
    assert oi.shape == (20,) and np.ndim(on) == 0 and on == count[0] and _same(oi[None], idx[:1])
    assert _same(multi_a_filter(c["rows"][0], oi)[None], amp[:1])


@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_book_through_the_gufuncs_with_device_arrays(emulated, loop):
    """rows, lists, ratios and outputs stay on the device; the packed list goes from one call to the next without leaving it"""
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import multi_a_filter, peak_snr_threshold

    T = pc.LOOPS[loop]
    for index, (c, idx, count, amp, fatal) in enumerate(_of_loop(emulated, loop)):
        if index % 3 and not c["key"].startswith("named"):
            continue
        R = _row_count(c, index + 2)
        m = c["m"]
        dev = [DeviceArray.from_numpy(np.ascontiguousarray(pc.tile_rows(c[k], R))) for k in ("rows", "lists", "ratio")]
        oi, on = DeviceArray.from_numpy(np.full((R, m), SENTINEL, T)), DeviceArray.from_numpy(np.full(R, 77, np.uint32))
        got = peak_snr_threshold(dev[0], dev[1], dev[2], c["width"], oi, on)
        assert got[0] is oi and got[1] is on
        assert np.array_equal(on.to_numpy(), pc.tile_rows(count, R)) and _same(oi.to_numpy(), pc.tile_rows(idx, R)), c["key"]
        if amp is not None and not fatal.any():
            oa = DeviceArray.from_numpy(np.full((R, m), SENTINEL, T))
            assert multi_a_filter(dev[0], oi, oa) is oa and _same(oa.to_numpy(), pc.tile_rows(amp, R)), c["key"]
            oa.free()
        for d in dev + [oi, on]:
            d.free()


def test_a_fractional_position_names_its_row_and_leaves_the_others_right():
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import multi_a_filter

    for T in pc.LOOPS.values():
        rng = np.random.default_rng(3)
        w = rng.normal(0, 1, (9, 65)).astype(T)
        vt = np.tile(np.array([3, 64, np.nan, 0, 17], T), (9, 1))
        want, _ = pc.emulate_pickoff(w, vt, T)
        vt[6, 3] = 10.5
        d, dv, out = DeviceArray.from_numpy(w), DeviceArray.from_numpy(vt), DeviceArray.from_numpy(np.full((9, 5), SENTINEL, T))
        with pytest.raises(DSPFatal, match="^fixed_time_pickoff requires integer t_in when using mode 'i'\n") as e:
            multi_a_filter(d, dv, out)
        assert e.value.wf_range == range(6, 7)
        got = out.to_numpy()
        keep = [r for r in range(9) if r != 6]
        assert _same(got[keep], want[keep]) and _same(got[6, [0, 1, 2, 4]], want[6, [0, 1, 2, 4]]) and np.isnan(got[6, 3])
        for x in (d, dv, out):
            x.free()
    with pytest.raises(DSPFatal, match="^The length of your return array must be smaller than the length of your waveform"):
        multi_a_filter(np.zeros((2, 5), np.float32), np.zeros((2, 5), np.float32))


# ---------------------------------------------------------------------------------------------------------------- 2. the C entries
def _block(a, off, stride, fill):
    """the rows of ``a`` in a block: the first element ``off`` in, rows ``stride`` apart, ``fill`` everywhere else"""
    R, n = a.shape
    block = np.full(8 + off + R * stride, fill, dtype=a.dtype)
    block[off:off + R * stride].reshape(R, stride)[:, :n] = a
    return block


def _check_block(got, want, off, stride, fill, what):
    R, n = want.shape
    body = got[off:off + R * stride].reshape(R, stride)
    assert _same(np.ascontiguousarray(body[:, :n]), want), (what, _diff(np.ascontiguousarray(body[:, :n]), want))
    assert (got[:off] == fill).all() and (body[:, n:] == fill).all() and (got[off + R * stride:] == fill).all(), what  # the canaries


@pytest.mark.parametrize("rows_type", [np.float32, np.int16, np.uint16, np.float64])
def test_layouts_through_the_c_entries_with_canaries(emulated, rows_type):
    """rows n + 0 .. 3 apart from an element 0 .. 3 past a 16-byte boundary (an offset view, a strided view), lists and outputs likewise: 16-byte
    loads in the streaming pass where start and stride allow, a sample per lane otherwise, and nothing but the m entries of every output row
    and the count of every row written"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.gufunc import run

    L = _lib.lib()
    loop = "f64" if rows_type is np.float64 else "f32"
    T = pc.LOOPS[loop]
    esz, isz = np.dtype(T).itemsize, np.dtype(rows_type).itemsize
    loop_code, code = _lib.F32 if T is np.float32 else _lib.F64, getattr(_lib, CODES[np.dtype(rows_type)])
    integer = np.dtype(rows_type).kind in "iu"
    vectors = set()
    for index, (c, idx, count, amp, fatal) in enumerate(_of_loop(emulated, loop)):
        if not c["key"].startswith("named") and (c["n"] not in (3, 64, 65, 1003) or c["m"] in (2, 63)):
            continue
        R = _row_count(c, index)
        n, m = c["n"], c["m"]
        w, lists, ratio = pc.tile_rows(c["rows"], R), pc.tile_rows(c["lists"], R), pc.tile_rows(c["ratio"], R)
        if integer:
            w = pc.integer_rows(w, rows_type)
            want_idx, want_n, _ = pc.emulate_picker(w, lists, ratio, c["width"], T)
            want_amp, want_fatal = pc.emulate_pickoff(w, want_idx, T) if m < n else (None, None)
        else:
            want_idx, want_n = pc.tile_rows(idx, R), pc.tile_rows(count, R)
            want_amp, want_fatal = (pc.tile_rows(amp, R), pc.tile_rows(fatal, R)) if amp is not None else (None, None)
        w = w.astype(rows_type)
        if index % 3 == 0:  # rows back to back from a 16-byte boundary: whole vectors where n is
            in_off, in_stride, l_off, l_stride, off, out_stride = 0, n, 0, m, 0, m
        else:
            in_off, in_stride = index % 4, n + (index // 4) % 4
            l_off, l_stride = (index // 3) % 3, m + (index // 5) % 3
            off, out_stride = (index // 2) % 4, m + (index // 3) % 3
        vectors.add(in_off * isz % 16 == 0 and in_stride * isz % 16 == 0 and n * isz % 16 == 0)
        d = DeviceArray.from_numpy(_block(w, in_off, in_stride, 77))
        dl = DeviceArray.from_numpy(_block(lists.astype(T), l_off, l_stride, T(5)))
        dr = DeviceArray.from_numpy(ratio.astype(T))
        oi = DeviceArray.from_numpy(np.full(8 + off + R * out_stride, SENTINEL, dtype=T))
        oa = DeviceArray.from_numpy(np.full(8 + off + R * out_stride, SENTINEL, dtype=T))
        on = DeviceArray.from_numpy(np.full(R + 4, 77, np.uint32))
        assert d.ptr % 16 == 0 and oi.ptr % 16 == 0
        run(L.dsp_peak_snr_threshold_rows, "peak_snr_threshold", d.ptr + in_off * isz, code, R, n, in_stride, loop_code, dl.ptr + l_off * esz, m, l_stride,
            dr.ptr, 0.0, float(c["width"]), oi.ptr + off * esz, out_stride, on.ptr)
        got_n = on.to_numpy()
        assert np.array_equal(got_n[:R], want_n) and (got_n[R:] == 77).all(), (rows_type, c["key"], R)
        _check_block(oi.to_numpy(), want_idx, off, out_stride, SENTINEL, (rows_type, c["key"], R))
        if want_amp is not None and not want_fatal.any():  # the pick-off reads the packed list where the picker wrote it
            run(L.dsp_multi_a_filter_rows, "multi_a_filter", d.ptr + in_off * isz, code, R, n, in_stride, loop_code, oi.ptr + off * esz, m, out_stride,
                oa.ptr + off * esz, out_stride)
            _check_block(oa.to_numpy(), want_amp, off, out_stride, SENTINEL, (rows_type, c["key"], R))
        assert d.to_numpy().tobytes() == _block(w, in_off, in_stride, 77).tobytes()  # (the rows are read, never written)
        for x in (d, dl, dr, oi, oa, on):
            x.free()
    assert vectors == {True, False}
    # a constant ratio, an empty list (nothing launched, nothing written)
    c, idx, count, _amp, _fatal = emulated[f"sweep_{loop}_n65_m20_w10"]
    w = c["rows"][:1].astype(rows_type) if not integer else pc.integer_rows(c["rows"][:1], rows_type)
    want_idx, want_n, _ = pc.emulate_picker(w, c["lists"][:1], 0.8, 10, T)
    d, dl = DeviceArray.from_numpy(w), DeviceArray.from_numpy(c["lists"][:1].copy())
    oi, on = DeviceArray.from_numpy(np.full((1, 20), SENTINEL, T)), DeviceArray.from_numpy(np.full(1, 77, np.uint32))
    run(L.dsp_peak_snr_threshold_rows, "peak_snr_threshold", d.ptr, code, 1, 65, 65, loop_code, dl.ptr, 20, 20, None, 0.8, 10.0, oi.ptr, 20, on.ptr)
    assert _same(oi.to_numpy(), want_idx) and np.array_equal(on.to_numpy(), want_n)
    run(L.dsp_peak_snr_threshold_rows, "peak_snr_threshold", d.ptr, code, 1, 65, 65, loop_code, dl.ptr, 0, 0, None, 0.8, 10.0, oi.ptr, 0, on.ptr)
    run(L.dsp_multi_a_filter_rows, "multi_a_filter", d.ptr, code, 1, 65, 65, loop_code, dl.ptr, 0, 0, oi.ptr, 0)
    assert _same(oi.to_numpy(), want_idx) and np.array_equal(on.to_numpy(), want_n)
    for x in (d, dl, oi, on):
        x.free()


# ---------------------------------------------------------------------------------------------------------------- 3. the fused launch
def _fused(loop, c, R, store_list, ratio_column):
    """LOAD, LOAD, PEAK_SNR_THRESHOLD, MULTI_A_FILTER, [STORE,] STORE, STORE_SCALAR as one launch: (idx_out or None, amplitudes, count)"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray, sync

    T = pc.LOOPS[loop]
    n, m = c["n"], c["m"]
    w, lists, ratio = pc.tile_rows(c["rows"], R), pc.tile_rows(c["lists"], R), pc.tile_rows(c["ratio"], R)
    chain = Chain(pc.program(n, m, w.dtype, T, amp=True, store_list=store_list, ratio="column" if ratio_column else float(ratio[0]), width=float(c["width"])),
                  compute_dtype=T)
    assert chain.kernel_name == pc.KERNEL and chain.geometry(R) == {"lds_bytes_per_wave": 0, "waves_per_block": 4, "blocks": -(-R // 4)}
    dev = {"w": DeviceArray.from_numpy(np.ascontiguousarray(w)), "list": DeviceArray.from_numpy(np.ascontiguousarray(lists)),
           "va_max": DeviceArray.from_numpy(np.full((R, m), SENTINEL, T)), "count": DeviceArray.from_numpy(np.full(R, 77, np.uint32))}
    if store_list:
        dev["idx_out"] = DeviceArray.from_numpy(np.full((R, m), SENTINEL, T))
    if ratio_column:
        dev["ratio"] = DeviceArray.from_numpy(np.ascontiguousarray(ratio))
    chain.execute(dev, R)
    sync()
    chain.check()
    got = (dev["idx_out"].to_numpy() if store_list else None, dev["va_max"].to_numpy(), dev["count"].to_numpy())
    chain.close()
    for d in dev.values():
        d.free()
    return got


@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_fused_launch_equals_the_emulation_and_the_two_calls_apart(emulated, loop):
    from dspeed_amd.processors import multi_a_filter, peak_snr_threshold

    T = pc.LOOPS[loop]
    launches = 0
    for index, (c, idx, count, amp, fatal) in enumerate(_of_loop(emulated, loop)):
        if amp is None or (index % 2 and not c["key"].startswith("named")):
            continue
        c, idx, count, amp = _without_fatal(c, idx, count, amp, fatal)
        R = _row_count(c, index + 1)
        same_ratio = bool((c["ratio"] == c["ratio"][0]).all())
        for store_list in (True, False):
            got_idx, got_amp, got_n = _fused(loop, c, R, store_list, ratio_column=not same_ratio or index % 4 == 0)
            assert np.array_equal(got_n, pc.tile_rows(count, R)), (c["key"], store_list)
            assert _same(got_amp, pc.tile_rows(amp, R)), (c["key"], store_list, _diff(got_amp, pc.tile_rows(amp, R)))
            assert got_idx is None or _same(got_idx, pc.tile_rows(idx, R)), (c["key"], store_list)
            launches += 1
    assert launches > 100
    c, idx, count, amp, _fatal = emulated[f"sweep_{loop}_n257_m20_w10"]
    oi, on = peak_snr_threshold(c["rows"], c["lists"], c["ratio"], 10)
    assert _same(multi_a_filter(c["rows"], oi), amp) and _same(oi, idx) and np.array_equal(on, count)  # apart: the same bits


def test_the_fused_launch_reports_a_fractional_candidate_with_its_row():
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray, sync
    from dspeed_amd.errors import DSPFatal

    (c,) = [c for c in pc.named_cases("f32") if "half-integer-kept" in c["names"]]
    r = c["names"].index("half-integer-kept")
    chain = Chain(pc.program(c["n"], c["m"], np.float32, np.float32, amp=True, ratio="column", width=float(c["width"])))
    R = len(c["rows"])
    dev = {"w": DeviceArray.from_numpy(c["rows"]), "list": DeviceArray.from_numpy(c["lists"]), "ratio": DeviceArray.from_numpy(c["ratio"]),
           "idx_out": DeviceArray((R, c["m"]), np.float32), "va_max": DeviceArray((R, c["m"]), np.float32), "count": DeviceArray((R,), np.uint32)}
    chain.execute(dev, R)
    sync()
    with pytest.raises(DSPFatal, match="fixed_time_pickoff requires integer t_in when using mode 'i'") as e:
        chain.check()
    fractional = [k for k, nm in enumerate(c["names"]) if nm in ("half-integer-kept", "half-integer-truncated-not-rounded", "fraction-truncated-not-rounded")]
    assert r in fractional and e.value.wf_range.start in fractional
    idx, count, _ = pc.emulate_picker(c["rows"], c["lists"], c["ratio"], c["width"], np.float32)
    assert _same(dev["idx_out"].to_numpy(), idx) and np.array_equal(dev["count"].to_numpy(), count)  # the picker's part is whole
    chain.close()
    for d in dev.values():
        d.free()


# ---------------------------------------------------------------------------------------------------------------- 4. the recipe
M = "dspeed.processors"
PICK = "trigger_pos, no_out"


def _book_recipe(width, fused):
    amp_of = "waveform" if fused else "waveform[0:]"
    return {PICK: {"function": "peak_snr_threshold", "module": f"{M}.peak_snr_threshold",
                   "args": ["waveform", "cands", "ratios", width, "trigger_pos(vector_len=no_out)", "no_out"]},
            "energies": {"function": "multi_a_filter", "module": f"{M}.multi_a_filter", "args": [amp_of, "trigger_pos", "energies(vector_len=len(trigger_pos))"]}}


def test_the_book_through_a_recipe(emulated):
    """the float32 book's rows, lists and ratios as columns of the table; the declarations name no length"""
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    chains = 0
    for index, (c, idx, count, amp, fatal) in enumerate(_of_loop(emulated, "f32")):
        if amp is None or (index % 4 and not c["key"].startswith("named")):
            continue
        c, idx, count, amp = _without_fatal(c, idx, count, amp, fatal)
        R = _row_count(c, index)
        table = {"waveform": WaveformInput(np.ascontiguousarray(pc.tile_rows(c["rows"], R)), 16.0), "cands": np.ascontiguousarray(pc.tile_rows(c["lists"], R)),
                 "ratios": np.ascontiguousarray(pc.tile_rows(c["ratio"], R))}
        outputs = ["energies", "trigger_pos", "no_out"] if index % 8 else ["energies"]
        chain, _, out = build_processing_chain({"outputs": outputs, "processors": _book_recipe(c["width"], fused=True)}, table)
        chain.execute()
        assert [kernel for _what, kernel in chain.kernels()].count(pc.KERNEL) == 1 and len(chain._stages) == 1
        assert out["no_out"].dtype == np.uint32 and np.array_equal(out["no_out"], pc.tile_rows(count, R)), c["key"]
        assert _same(np.asarray(out["energies"]), pc.tile_rows(amp, R)), (c["key"], _diff(np.asarray(out["energies"]), pc.tile_rows(amp, R)))
        assert "trigger_pos" not in outputs or _same(np.asarray(out["trigger_pos"]), pc.tile_rows(idx, R)), c["key"]
        chains += 1
    assert chains > 30


# ---------------------------------------------------------------------------------------------------------------- 5. the SiPM fragment
LAG, BINS, LISTS, WIDTH, RATIO = 5, 100, 20, 10, 0.8
PEAKS = "vt_max_candidate_out, vt_min_out, n_max_out, n_min_out"


def _sipm_rows(n_rows=36, n=1000):
    """a pulse train on noise on a pedestal: one to six pulses a row with an undershoot behind each, a few rows of noise alone"""
    rng = np.random.default_rng(11)
    t = np.arange(n)
    w = 1000 + rng.normal(0, 2.0, (n_rows, n))
    for r in range(n_rows):
        for _ in range(r % 7):
            p, a = rng.integers(30, n - 40), rng.uniform(60, 400)
            w[r] += a * (t >= p) * np.exp(-(t - p) / 12.0) - 0.3 * a * (t >= p + 15) * np.exp(-(t - p - 15) / 25.0)
    return np.rint(w).astype(np.uint16)


def _sipm_recipe():
    return {
        "wf_gaus": {"function": "reflected_convolve_wf", "module": f"{M}.convolutions", "args": ["waveform", "db.kernel", "wf_gaus"], "unit": "ADC"},
        "curr": {"function": "avg_current", "module": f"{M}.moving_windows", "args": ["wf_gaus", LAG, f"curr(len(wf_gaus)-{LAG}, period=waveform.period)"], "unit": "ADC"},
        "hist_weights, hist_borders": {"function": "histogram", "module": f"{M}.histogram", "args": ["curr", f"hist_weights({BINS})", f"hist_borders({BINS + 1})"],
                                       "unit": ["none", "ADC"]},
        "fwhm, idx_out_c, max_out": {"function": "histogram_stats", "module": M, "args": ["hist_weights", "hist_borders", "idx_out_c", "max_out", "fwhm", "np.nan"],
                                     "unit": ["ADC", "non", "ADC"]},
        PEAKS: {"function": "get_multi_local_extrema", "module": f"{M}.get_multi_local_extrema",
                "args": ["curr", 5, 0.1, 1, "3*fwhm", 0, f"vt_max_candidate_out({LISTS}, vector_len=n_max_out)", f"vt_min_out({LISTS}, vector_len=n_min_out)",
                         "n_max_out", "n_min_out"], "unit": ["ns", "ns", "none", "none"]},
        PICK: {"function": "peak_snr_threshold", "module": f"{M}.peak_snr_threshold",
               "args": ["curr", "vt_max_candidate_out", RATIO, WIDTH, "trigger_pos(vector_len=no_out)", "no_out"], "unit": ["ns", "none"]},
        "energies": {"function": "multi_a_filter", "module": f"{M}.multi_a_filter", "args": ["curr", "trigger_pos", "energies(vector_len=len(trigger_pos))"],
                     "unit": ["ADC"]},
    }


def _sipm_kernel():
    from dspeed_amd.processors import gaussian_filter1d

    return gaussian_filter1d(np.float32(1), np.float32(4), np.empty(9, np.float32))


def _sipm_model(w, kernel):
    """the emulations of each step, chained on the CPU"""
    import extrema_cases as xc
    import histogram_cases as hc
    import reflect_cases as rc

    F32 = np.float32
    curr = rc.avg_current(rc.emulate(w, kernel, F32), LAG)
    cands, n_max = np.empty((len(w), LISTS), F32), np.empty(len(w), np.uint32)
    for r, row in enumerate(curr):
        weights, borders = hc.model_histogram(row, BINS, F32, 1)
        _mode, _max, fwhm = hc.model_stats(weights, borders, np.nan, F32)
        cands[r], _vt_min, n_max[r], _n_min = xc.model(row, 5, 0.1, 1, F32(3) * F32(fwhm), 0, LISTS, F32, 1)
    idx, count, _ = pc.emulate_picker(curr, cands, RATIO, WIDTH, F32)
    amp, fatal = pc.emulate_pickoff(curr, idx, F32)
    assert not fatal.any()
    return curr, cands, n_max, idx, count, amp


def test_the_sipm_fragment_on_a_pulse_train_equals_the_chained_emulations():
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    w, kernel = _sipm_rows(), _sipm_kernel()
    curr, cands, n_max, idx, count, amp = _sipm_model(w, kernel)
    assert (n_max > count).any() and (count > 0).sum() > 20 and (count == 0).any() and len(set(count.tolist())) > 3  # the rows are not trivial
    chain, _, out = build_processing_chain({"outputs": ["energies", "trigger_pos", "curr", "n_max_out"], "processors": _sipm_recipe()},
                                           {"waveform": WaveformInput(w, 16.0)}, db_dict={"kernel": kernel})
    chain.execute()
    assert [kernel for _what, kernel in chain.kernels()].count(pc.KERNEL) == 1
    assert _same(np.asarray(out["curr"]), curr) and np.array_equal(out["n_max_out"], n_max)  # the steps ahead, for the record
    assert out["no_out"].dtype == np.uint32 and np.array_equal(out["no_out"], count)
    assert _same(np.asarray(out["energies"]), amp), _diff(np.asarray(out["energies"]), amp)
    assert _same(np.asarray(out["trigger_pos"]), (idx * np.float32(16.0)).astype(np.float32))  # ns at the output, sample indices inside
    assert chain.vector_lens["energies"] == "no_out" and chain.vector_lens["trigger_pos"] == "no_out"


def test_build_dsp_delivers_both_outputs_clipped_to_their_counts():
    from lgdo_standins import Table, WaveformTable

    from dspeed_amd import lgdo_io
    from dspeed_amd.build_dsp import build_dsp

    w, kernel = _sipm_rows(), _sipm_kernel()
    _curr, _cands, _n_max, idx, count, amp = _sipm_model(w, kernel)
    res = build_dsp(Table(waveform=WaveformTable(w, 16.0, np.zeros(len(w)))), dsp_config={"outputs": ["energies", "trigger_pos"], "processors": _sipm_recipe()},
                    database={"kernel": kernel})
    for name, want in (("energies", amp), ("trigger_pos", (idx * np.float32(16.0)).astype(np.float32))):
        vov = res[name]
        flat, cum = vov.to_flat() if isinstance(vov, lgdo_io.RaggedColumn) else (np.asarray(vov.flattened_data.nda), np.asarray(vov.cumulative_length.nda))
        assert np.array_equal(cum, np.cumsum(count)) and np.array_equal(flat, np.concatenate([want[r, :k] for r, k in enumerate(count)])), name
