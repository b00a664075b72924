"""multi_time_point_thresh and time_over_threshold on the device (dsp_thresh.hip) against tests/golden/thresholds.npz (what
test_threshold_cases_cpu.py vouches for): every time and every count bit for bit -- through the gufuncs, the C entries and recipes."""
import ctypes as C

import numpy as np
import pytest

import golden_util
import threshold_cases as tc

pytestmark = pytest.mark.gpu
M = "dspeed.processors"


@pytest.fixture(scope="module")
def book():
    return golden_util.cases(tc.BOOK, kernel=tc.KERNEL)


def _same(got, want, what=""):
    got = got.to_numpy() if hasattr(got, "to_numpy") else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (what, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])


def _combos(c):
    return [(p, m) for p, m in map(tuple, c.params["combos"])]


def test_every_case_of_the_book_through_the_gufunc(book):
    """thresholds as an (rows, m) array with t_start a column, and -- the groups with one list and one start -- both as constants"""
    from dspeed_amd.processors import multi_time_point_thresh

    assert any(len(c["w"]) % 4 for c in book)  # a partial workgroup among the launches
    n_launches = 0
    for c in book:
        w, thr, ts = c["w"], c["thr"], c["ts"]
        for pol, mode in _combos(c):
            want = c[tc.key(pol, mode)]
            out = np.full(want.shape, -7, dtype=c.dtype)
            if c.params["shared"]:
                ret = multi_time_point_thresh(w, thr[0], ts[0], pol, ord(mode), out)
            else:
                ret = multi_time_point_thresh(w, thr, ts, pol, mode, out)
            assert ret is out
            _same(out, want, (c.name, pol, mode))
            n_launches += 1
    assert n_launches == 8 * len(book)


def test_time_over_threshold_through_the_gufunc_and_the_c_entry(book):
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import time_over_threshold

    for c in book:
        w, thr = c["w"], c["tot_thr"]
        _same(time_over_threshold(w, thr), c["tot"], c.name)
        r = len(w) // 2  # one row, a constant threshold
        _same(np.asarray(time_over_threshold(w[r], thr[r]), dtype=c.dtype), c["tot"][r], (c.name, "one row"))
    # the C entry: uint16 rows 1003 elements apart from an odd element on, a constant threshold
    c = next(c for c in book if c.name.startswith("u16_n1000"))
    w = c["w"]
    block = np.zeros(len(w) * 1003 + 1, dtype=np.uint16)
    for k in range(len(w)):
        block[1 + k * 1003: 1 + k * 1003 + 1000] = w[k]
    d, out, row = DeviceArray.from_numpy(block), DeviceArray.from_numpy(np.full(len(w), -7, dtype=np.float32)), C.c_int64(-1)
    rc = _lib.lib().dsp_time_over_threshold_f32(d.ptr + 2, _lib.U16, len(w), 1000, 1003, None, 101.0, out.ptr, None, C.byref(row))
    assert rc == 0, _lib.last_error()
    _same(out, (w > 101).sum(axis=1).astype(np.float32), "C entry")


def test_every_case_of_the_book_through_the_c_entry(book):
    """the rows, lists and starts of a group sent once; one call per (polarity, mode): lists m apart with t_start a column, or one list
    (stride 0) with a constant t_start"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray

    L, row = _lib.lib(), C.c_int64(-1)
    for c in book:
        sfx, code = ("f32", {"f32": _lib.F32, "i16": _lib.I16, "u16": _lib.U16}[c.params["rows_type"]]) if c.tag == "f32" else ("f64", _lib.F64)
        fn = getattr(L, f"dsp_multi_time_point_thresh_{sfx}")
        n_wf, n, m = len(c["w"]), c.params["n"], c.params["m"]
        d, dl, dts = DeviceArray.from_numpy(c["w"]), DeviceArray.from_numpy(c["thr"]), DeviceArray.from_numpy(c["ts"])
        out = DeviceArray((n_wf, m), c.dtype)
        for pol, mode in _combos(c):
            if c.params["shared"]:
                rc = fn(d.ptr, code, n_wf, n, n, dl.ptr, m, 0, None, float(c["ts"][0]), pol, ord(mode), out.ptr, m, None, C.byref(row))
            else:
                rc = fn(d.ptr, code, n_wf, n, n, dl.ptr, m, m, dts.ptr, 0.0, pol, ord(mode), out.ptr, m, None, C.byref(row))
            assert rc == 0, _lib.last_error()
            _same(out, c[tc.key(pol, mode)], (c.name, pol, mode))


def test_every_case_of_the_float32_loop_through_a_recipe(book):
    """multi_time_point_thresh and time_over_threshold as a recipe's processors on the groups' rows: a list per event is a two-dimensional
    input column and t_start a column; one list for all is a list literal with a constant t_start (the float64 loop is refused in recipes)"""
    from dspeed_amd.processing_chain import build_processing_chain

    n_chains = 0
    for c in [c for c in book if c.tag == "f32"]:
        tb = {"waveform": c["w"], "lists": c["thr"], "start": c["ts"], "level": c["tot_thr"]}
        for pol, mode in _combos(c):
            if c.params["shared"]:
                args = ["waveform", str([float(v) for v in c["thr"][0]]), float(c["ts"][0]), pol, f"'{mode}'", "t_out"]
            else:
                args = ["waveform", "lists", "start", pol, f"'{mode}'", "t_out"]
            procs = {"t_out": {"function": "multi_time_point_thresh", "module": f"{M}.time_point_thresh", "args": args},
                     "n_over": {"function": "time_over_threshold", "module": f"{M}.time_over_threshold", "args": ["waveform", "level", "n_over"]}}
            chain, _, out = build_processing_chain({"outputs": ["t_out", "n_over"], "processors": procs}, tb)
            chain.execute()
            assert [k for _w, k in chain.kernels()].count("dsp_thresh_kernel") == 2
            _same(out["t_out"], c[tc.key(pol, mode)], (c.name, pol, mode))
            _same(out["n_over"], c["tot"], (c.name, "time_over_threshold"))
            n_chains += 1
    assert n_chains >= 100


def test_a_rise_time_recipe_on_uint16_rows_with_a_time_unit():
    """24 rows of 1000 uint16 samples: bl_subtract -> min_max_norm -> the 10 / 50 / 90 % times from the maximum backwards, in ns, and the time
    over half the maximum, in ns; against the model on the rows the recipe itself hands to the stage (wf_norm, the first maximum)"""
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    w = tc.recipe_rows()
    assert w.shape == (24, 1000) and w.dtype == np.uint16
    bl = np.random.default_rng(6).uniform(990, 1010, 24).astype(np.float32)
    outs = ["tps", "t_sat", "wf_norm", "wf_max", "t_hi"]
    chain, _, out = build_processing_chain({"outputs": outs, "processors": tc.rise_time_recipe(unit="ns")}, {"waveform": WaveformInput(w, 16.0), "bl": bl})
    chain.execute()
    kernels = [k for _w, k in chain.kernels()]
    assert kernels.count("dsp_thresh_kernel") == 2
    norm = out["wf_norm"]
    assert np.array_equal(out["t_hi"], np.argmax(norm, axis=1).astype(np.float32))
    thr = np.float32([0.1, 0.5, 0.9])
    want = np.stack([tc.model(norm[r], thr, out["t_hi"][r], 1, "l", np.float32) for r in range(24)])
    assert np.isfinite(want).all() and (np.diff(want, axis=1) > 0).all() and (want != np.floor(want)).any()
    _same(out["tps"], want * np.float32(16.0), "tps in ns")
    blsub = w.astype(np.float32) - bl[:, None]
    count = (blsub > np.float32(0.5) * out["wf_max"][:, None]).sum(axis=1).astype(np.float32)
    assert count.min() > 100
    _same(out["t_sat"], count * np.float32(16.0), "t_sat in ns")


def test_a_threshold_read_off_a_waveform_the_program_computes():
    """time_over_threshold of the input rows above half the maximum of the baseline-subtracted waveform: min_max's results are written to
    memory ahead of the stage, and leave the recipe as outputs all the same"""
    from dspeed_amd.processing_chain import build_processing_chain

    w = tc.recipe_rows()
    bl = np.random.default_rng(6).uniform(990, 1010, 24).astype(np.float32)
    chain, _, out = build_processing_chain({"outputs": ["n_over", "wf_max", "tp_max"], "processors": tc.over_half_recipe()}, {"waveform": w, "bl": bl})
    chain.execute()
    blsub = w.astype(np.float32) - bl[:, None]
    _same(out["wf_max"], blsub.max(axis=1), "wf_max")
    _same(out["tp_max"], np.argmax(blsub, axis=1).astype(np.float32), "tp_max")
    _same(out["n_over"], (w.astype(np.float32) > np.float32(0.5) * out["wf_max"][:, None]).sum(axis=1).astype(np.float32), "n_over")
    assert 0 < out["n_over"].min() and (out["n_over"] < 1000).sum() >= 8  # (rows whose half maximum lies below the pedestal are above it throughout)


def test_one_dimensional_and_strided_arguments(book):
    from dspeed_amd.processors import multi_time_point_thresh

    c = next(c for c in book if c.name == "f32_n1000_m7")
    pol, mode = _combos(c)[0]
    want = c[tc.key(pol, mode)]
    for r in (0, 5):  # one row: 1-D rows, thresholds and result; the result allocated
        got = multi_time_point_thresh(c["w"][r], c["thr"][r], c["ts"][r], pol, mode)
        _same(got, want[r], ("1-D", r))
    # every second row of a block twice as wide, every second threshold of a list twice as long
    wide = np.zeros((2 * len(c["w"]), 2000), dtype=np.float32)
    wide[::2, :1000] = c["w"]
    lists = np.zeros((len(c["w"]), 14), dtype=np.float32)
    lists[:, ::2] = c["thr"]
    out = np.full((len(c["w"]), 14), -7, dtype=np.float32)
    multi_time_point_thresh(wide[::2, :1000], lists[:, ::2], c["ts"], pol, mode, out[:, ::2])
    _same(np.ascontiguousarray(out[:, ::2]), want, "strided")
    assert (out[:, 1::2] == -7).all()
    # no threshold: an empty result
    got = multi_time_point_thresh(c["w"], np.empty((len(c["w"]), 0), np.float32), c["ts"], pol, mode)
    assert got.shape == (len(c["w"]), 0) and got.dtype == np.float32


def test_c_abi_entries_on_unaligned_strided_rows(book):
    """dsp_multi_time_point_thresh_f32 called directly: int16 rows 1003 elements apart from an odd element on (the one-sample-per-lane
    kernel), lists of thresholds 9 apart, times 11 apart; then one list for every row (stride 0) and a constant t_start; the float64 entry"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray

    L, row = _lib.lib(), C.c_int64(-1)
    c = next(c for c in book if c.name.startswith("i16_n1000"))
    w, m, n_wf = c["w"], c.params["m"], len(c["w"])
    block = np.zeros(n_wf * 1003 + 1, dtype=np.int16)
    for k in range(n_wf):
        block[1 + k * 1003: 1 + k * 1003 + 1000] = w[k]
    lists = np.zeros((n_wf, m + 2), dtype=np.float32)
    lists[:, :m] = c["thr"]
    d, dl, dts = DeviceArray.from_numpy(block), DeviceArray.from_numpy(lists), DeviceArray.from_numpy(c["ts"])
    for pol, mode in _combos(c)[:4]:
        out = DeviceArray.from_numpy(np.full((n_wf, m + 4), -7, dtype=np.float32))
        if c.params["shared"]:
            rc = L.dsp_multi_time_point_thresh_f32(d.ptr + 2, _lib.I16, n_wf, 1000, 1003, dl.ptr, m, 0, None, float(c["ts"][0]), pol, ord(mode), out.ptr, m + 4, None, C.byref(row))
        else:
            rc = L.dsp_multi_time_point_thresh_f32(d.ptr + 2, _lib.I16, n_wf, 1000, 1003, dl.ptr, m, m + 2, dts.ptr, 0.0, pol, ord(mode), out.ptr, m + 4, None, C.byref(row))
        assert rc == 0, _lib.last_error()
        _same(out.to_numpy()[:, :m], c[tc.key(pol, mode)], (pol, mode))
        assert (out.to_numpy()[:, m:] == -7).all()
    c = next(c for c in book if c.name.startswith("f64_n129"))
    w, m, n_wf = np.ascontiguousarray(c["w"]), c.params["m"], len(c["w"])
    d, dl, dts = DeviceArray.from_numpy(w), DeviceArray.from_numpy(np.ascontiguousarray(c["thr"])), DeviceArray.from_numpy(c["ts"])
    pol, mode = _combos(c)[-1]
    out = DeviceArray((n_wf, m), np.float64)
    if c.params["shared"]:
        rc = L.dsp_multi_time_point_thresh_f64(d.ptr, _lib.F64, n_wf, 129, 129, dl.ptr, m, 0, None, float(c["ts"][0]), pol, ord(mode), out.ptr, m, None, C.byref(row))
    else:
        rc = L.dsp_multi_time_point_thresh_f64(d.ptr, _lib.F64, n_wf, 129, 129, dl.ptr, m, m, dts.ptr, 0.0, pol, ord(mode), out.ptr, m, None, C.byref(row))
    assert rc == 0, _lib.last_error()
    _same(out, c[tc.key(pol, mode)], "f64")


@pytest.mark.parametrize("n", [8192, 8190])
def test_sixteen_rows_through_the_vector_path_and_the_other(book, n):
    """8192 samples: whole 16-byte vectors; the same rows cut to 8190: a sample per lane.  Against the model (held against the reference
    by the CPU test) where no fixture has the length."""
    from dspeed_amd.processors import multi_time_point_thresh, time_over_threshold

    c = next(c for c in book if c.name.startswith("f32_n8192"))
    m = c.params["m"]
    w = np.ascontiguousarray(np.tile(c["w"], (2, 1))[:16, :n])
    thr, ts = np.tile(c["thr"], (2, 1))[:16], np.minimum(np.tile(c["ts"], 2)[:16], np.float32(n - 1))
    for pol, mode in ((1.0, "l"), (-1.0, "l"), (3.0, "r")):
        want = np.stack([tc.model(w[r], thr[r], ts[r], pol, mode, np.float32) for r in range(16)])
        if n == 8192 and not c.params["shared"] and (pol, mode) in _combos(c):
            _same(want[:8], c[tc.key(pol, mode)], "model")
        _same(multi_time_point_thresh(w, thr, ts, pol, mode), want, (n, pol, mode))
        assert np.isfinite(want).any(axis=1).sum() >= 4
    count = np.array([tc.model_time_over_threshold(w[r], 1.0, np.float32) for r in range(16)], dtype=np.float32)  # (NaN for a row with a NaN)
    assert np.isfinite(count).sum() >= 8
    _same(time_over_threshold(w, np.float32(1.0)), count, "count")


def test_the_reference_s_checks_and_the_refusals():
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import multi_time_point_thresh

    w = np.arange(40, dtype=np.float32).reshape(4, 10)
    thr = np.array([2.5, 7.5], dtype=np.float32)
    _same(multi_time_point_thresh(w, thr[None, :] + w[:, :1], 5, 1, "i"), np.tile(np.float32([2, 7]), (4, 1)))
    with pytest.raises(DSPFatal, match="polarity cannot be 0"):
        multi_time_point_thresh(w, thr, 5, 0, "i")
    with pytest.raises(DSPFatal, match="Unrecognized interpolation mode"):
        multi_time_point_thresh(w, thr, 5, 1, "h")
    with pytest.raises(NotImplementedError, match="at most 64 thresholds"):
        multi_time_point_thresh(w, np.zeros(65, np.float32), 5, 1, "i")
    with pytest.raises(NotImplementedError, match="polarity is a constant"):
        multi_time_point_thresh(w, thr, 5, np.array([1, 1, -1, 1]), "i")
    with pytest.raises(NotImplementedError, match="float64 loop takes float64 rows"):
        multi_time_point_thresh(w.astype(np.int32), thr.astype(np.float64), 5, 1, "i")
    # a start outside the row is a NaN row, for every row
    assert np.isnan(multi_time_point_thresh(w, thr, np.float32([-1, 10, np.nan, 1e9]), 1, "i")).all()
