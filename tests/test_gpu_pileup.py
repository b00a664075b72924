"""rc_cr2 and bi_level_zero_crossing_time_points on the device (dsp_pileup.hip): the whole book of tests/pileup_cases.py against its
emulation with numba's cube and the C library's exp -- every bit, both loops, filter rows, counts, lists and polarities --, through the
gufuncs and, for the layouts a gufunc call cannot make (padded strides, element offsets 0 .. 3 on both sides, a sentinel behind every
output row and list, int16 and uint16 rows), through the C entries; the fused launch against the two calls apart, with the row on which the
float64 state and its float32 rounding disagree about a threshold; the fatal paths."""
import numpy as np
import pytest

import pileup_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
CODES = {np.dtype(np.float32): "F32", np.dtype(np.int16): "I16", np.dtype(np.uint16): "U16", np.dtype(np.float64): "F64"}


def _same(got, want):
    return (got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
            and np.array_equal(np.signbit(got), np.signbit(want)))


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    idx = np.nonzero(bad)
    return int(bad.sum()), [i[:6].tolist() for i in idx], got[bad][:4], want[bad][:4]


def _want_filter(rows, tau, T):
    """the device's rule: the product cube, the pole from the C library's exp (the planner forms it on the host)"""
    return pc.emulate_rc_cr2(rows, tau, T, cube="product", exp="libm")


def _quiet(loop, n):
    """the filter's rows without the one it raises on"""
    keep = [k for k, f in enumerate(pc.FILTER_FAMILIES) if f not in pc.FILTER_FATAL]
    return pc.filter_rows(loop, n)[keep]


# ---------------------------------------------------------------------------------------------------------------- 1. the whole book
@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_filters_book_through_the_gufunc(loop):
    from dspeed_amd.processors import rc_cr2

    T = pc.LOOPS[loop]
    for index, (key, n, tau) in enumerate(pc.filter_cases(loop)):
        R = pc.ROW_COUNTS[index % len(pc.ROW_COUNTS)]
        w = pc.tile_rows(_quiet(loop, n), R)
        want, fatal = _want_filter(w, tau, T)
        assert not fatal.any()
        out = np.full((R, n), SENTINEL, dtype=T)
        assert rc_cr2(w, T(tau), out) is out
        assert _same(out, want), (key, R, _diff(out, want))
    w = _quiet(loop, 129)
    got = rc_cr2(w, 100)  # the output left out: a new array of the loop's type
    assert _same(got, _want_filter(w, 100, T)[0])
    one = rc_cr2(w[0], 100)  # a 1-D call
    assert one.shape == (129,) and _same(one[None], _want_filter(w[:1], 100, T)[0])


@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_walks_book_through_the_gufunc(loop):
    """every operand a value per row; then the first row of each case once more with constants, as a 1-D call"""
    from dspeed_amd.processors import bi_level_zero_crossing_time_points as walk

    T = pc.LOOPS[loop]
    over = 0
    for index, c in enumerate(pc.walk_cases(loop)):
        R = pc.ROW_COUNTS[index % len(pc.ROW_COUNTS)]
        w, pos, neg, gate, ts = (pc.tile_rows(c[k], R) for k in ("rows", "pos", "neg", "gate", "t_start"))
        want = pc.emulate_walk(w, pos, neg, gate, ts, c["m"], T)
        count, polarity, times = np.full(R, 77, np.uint32), np.full((R, c["m"]), SENTINEL, T), np.full((R, c["m"]), SENTINEL, T)
        got = walk(w, pos, neg, gate, ts, count, polarity, times)
        assert got[0] is count and got[1] is polarity and got[2] is times
        assert np.array_equal(count, want[0]), (c["key"], R, [c["names"][k % len(c["names"])] for k in np.flatnonzero(count != want[0])][:6])
        assert _same(polarity, want[1]) and _same(times, want[2]), (c["key"], R, _diff(times, want[2]))
        over += int((count > c["m"]).sum())
        for r in (0, 3):
            want1 = pc.emulate_walk(c["rows"][r], c["pos"][r], c["neg"][r], c["gate"][r], c["t_start"][r], c["m"], T)
            n1, p1, t1 = walk(c["rows"][r], float(c["pos"][r]), float(c["neg"][r]), float(c["gate"][r]), float(c["t_start"][r]), None,
                              np.empty(c["m"], T), np.empty(c["m"], T))
            assert int(n1) == int(want1[0][0]) and np.asarray(n1).dtype == np.uint32 and _same(p1[None], want1[1]) and _same(t1[None], want1[2]), (c["key"], r)
    assert over > 50


def test_the_two_rows_the_reference_counts_differently():
    from dspeed_amd.processors import bi_level_zero_crossing_time_points as walk

    for row, n, t, p in ((pc.SAMPLE0, 2, [2, 4], 0), (pc.SAMPLE0_TWIN, 3, [2, 4, 6], 1)):
        for T in pc.LOOPS.values():
            count, polarity, times = walk(np.array(row, T), 1, -1, 10, 0, None, np.empty(5, T), np.empty(5, T))
            assert count == n and list(times[:n]) == t and list(polarity[:n]) == [p] * n and np.isnan(times[n:]).all() and np.isnan(polarity[n:]).all()


# ---------------------------------------------------------------------------------------------------------------- 2. the C entries
def _blocks(w, loop, in_off, in_stride):
    block = np.full(8 + len(w) * in_stride, 77, dtype=w.dtype)
    block[in_off:in_off + len(w) * in_stride].reshape(len(w), in_stride)[:, :w.shape[1]] = w
    return block


@pytest.mark.parametrize("rows_type", [np.float32, np.int16, np.uint16, np.float64])
def test_layouts_through_the_c_entries_with_sentinels(rows_type):
    """rows n + 0 .. 3 apart from an element 0 .. 3 past a 16-byte boundary on the way in, likewise on the way out: 16-byte loads and stores
    where start and stride allow, an element per lane otherwise, and nothing but the n samples of every row and the m entries of every list
    written"""
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
    index = 0
    for n in pc.LENGTHS + (512,):
        for tau in (20, 100):
            index += 1
            base = pc.filter_rows(loop, n)[[pc.FILTER_FAMILIES.index("integer")]] if integer else _quiet(loop, n)
            R = pc.ROW_COUNTS[index % len(pc.ROW_COUNTS)]
            w = pc.tile_rows(base, R).astype(rows_type)
            want, _ = _want_filter(w, tau, T)
            if tau == 20:  # rows back to back from a 16-byte boundary: whole vectors where n is
                in_off, in_stride, off, out_stride = 0, n, 0, n
            else:
                in_off, in_stride = index % 4, n + (index // 4) % 4
                off, out_stride = (index // 2) % 4, n + (index // 3) % 3
            block = _blocks(w, loop, in_off, in_stride)
            blank = np.full(4 + R * out_stride + 8, SENTINEL, dtype=T)
            d, o = DeviceArray.from_numpy(block), DeviceArray.from_numpy(blank)
            assert o.ptr % 16 == 0 and d.ptr % 16 == 0
            vectors.add((in_off * isz % 16 == 0 and in_stride * isz % 16 == 0 and n * isz % 16 == 0, off * esz % 16 == 0 and out_stride * esz % 16 == 0))
            run(L.dsp_rc_cr2_rows, "rc_cr2", d.ptr + in_off * isz, code, R, n, in_stride, loop_code, float(T(tau)), o.ptr + off * esz, out_stride)
            got = o.to_numpy()
            body = got[off:off + R * out_stride].reshape(R, out_stride)
            assert _same(np.ascontiguousarray(body[:, :n]), want), (rows_type, n, tau, R, _diff(np.ascontiguousarray(body[:, :n]), want))
            assert (got[:off] == SENTINEL).all() and (body[:, n:] == SENTINEL).all() and (got[off + R * out_stride:] == SENTINEL).all(), (rows_type, n, tau)
            assert d.to_numpy().tobytes() == block.tobytes()  # (the rows are read, never written)
            d.free(), o.free()
    assert {v[0] for v in vectors} == {True, False} and {v[1] for v in vectors} == {True, False}
    # the walk: the same layouts on the way in; lists m + 0 .. 2 apart from an element 0 .. 3 on
    for index, c in enumerate(pc.walk_cases(loop)):
        if c["m"] == 30 and c["n"] not in (65, 257):
            continue
        R = pc.ROW_COUNTS[index % len(pc.ROW_COUNTS)]
        w, pos, neg, gate, ts = (pc.tile_rows(c[k], R) for k in ("rows", "pos", "neg", "gate", "t_start"))
        if integer:  # whole numbers in the type's range; a NaN or an infinity has no integer: those rows become 0 rows
            w = np.where(np.isfinite(w), np.rint(w), 0)
            w = np.abs(w) if rows_type is np.uint16 else w
        w = w.astype(rows_type)
        n, m = c["n"], c["m"]
        want = pc.emulate_walk(w, pos, neg, gate, ts, m, T)
        in_off, in_stride = index % 4, n + (index // 4) % 4
        off, out_stride = (index // 2) % 4, m + (index // 3) % 3
        block = _blocks(w, loop, in_off, in_stride)
        d = DeviceArray.from_numpy(block)
        lists = [DeviceArray.from_numpy(np.full(4 + R * out_stride + 8, SENTINEL, dtype=T)) for _ in range(2)]
        counts = DeviceArray.from_numpy(np.full(R + 4, 77, np.uint32))
        cols = [DeviceArray.from_numpy(np.ascontiguousarray(v, dtype=T)) for v in (pos, neg, gate, ts)]
        run(L.dsp_bi_level_zero_crossing_rows, "bi_level_zero_crossing_time_points", d.ptr + in_off * isz, code, R, n, in_stride, loop_code,
            cols[0].ptr, 0.0, cols[1].ptr, 0.0, cols[2].ptr, 0.0, cols[3].ptr, 0.0, counts.ptr, lists[0].ptr + off * esz, lists[1].ptr + off * esz, m, out_stride)
        got_n = counts.to_numpy()
        assert np.array_equal(got_n[:R], want[0]) and (got_n[R:] == 77).all(), (rows_type, c["key"], R)
        for dev, expect in zip(lists, want[1:]):
            got = dev.to_numpy()
            body = got[off:off + R * out_stride].reshape(R, out_stride)
            assert _same(np.ascontiguousarray(body[:, :m]), expect), (rows_type, c["key"], R, _diff(np.ascontiguousarray(body[:, :m]), expect))
            assert (got[:off] == SENTINEL).all() and (body[:, m:] == SENTINEL).all() and (got[off + R * out_stride:] == SENTINEL).all(), (rows_type, c["key"])
        for x in [d, counts] + lists + cols:
            x.free()


# ---------------------------------------------------------------------------------------------------------------- 3. fused against apart
def _fused(loop, w, tau, pos, neg, gate, ts, m, store_row, columns, subtract=None):
    """LOAD, [BL_SUBTRACT,] RC_CR2, BI_LEVEL_ZERO_CROSSING, [STORE,] STORE, STORE, STORE_SCALAR as one launch: (filtered rows or None, count,
    polarity, times); ``subtract``: a baseline for all rows, or an array of one per row"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray, sync

    T = pc.LOOPS[loop]
    R, n = w.shape
    per_row = isinstance(subtract, np.ndarray)
    chain = Chain(pc.program(n, w.dtype, T, walk=True, m=m, store_row=store_row, tau=float(T(tau)), columns=columns,
                             operands=(float(pos), float(neg), float(gate), float(ts)), subtract="column" if per_row else subtract), compute_dtype=T)
    assert chain.kernel_name == pc.KERNEL and chain.geometry(R)["blocks"] == -(-R // 64)
    dev = {"w": DeviceArray.from_numpy(w), "polarity": DeviceArray.from_numpy(np.full((R, m), SENTINEL, T)),
           "times": DeviceArray.from_numpy(np.full((R, m), SENTINEL, T)), "count": DeviceArray.from_numpy(np.full(R, 77, np.uint32))}
    if store_row:
        dev["out"] = DeviceArray.from_numpy(np.full((R, n), SENTINEL, T))
    if per_row:
        dev["bl"] = DeviceArray.from_numpy(subtract.astype(T))
    for k, (name, v) in enumerate(zip(("pos", "neg", "gate", "t_start"), (pos, neg, gate, ts))):
        if k in columns:
            dev[name] = DeviceArray.from_numpy(np.full(R, v, T))
    chain.execute(dev, R)
    sync()
    chain.check()
    got = (dev["out"].to_numpy() if store_row else None, dev["count"].to_numpy(), dev["polarity"].to_numpy(), dev["times"].to_numpy())
    chain.close()
    for d in dev.values():
        d.free()
    return got


@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_fused_launch_equals_the_two_calls_apart(loop):
    from dspeed_amd.processors import bi_level_zero_crossing_time_points as walk
    from dspeed_amd.processors import rc_cr2

    T = pc.LOOPS[loop]
    found = 0
    for index, f in enumerate(pc.FUSED):
        c = pc.fused_case(loop, *f)
        R = pc.ROW_COUNTS[index % len(pc.ROW_COUNTS)]
        w = pc.tile_rows(c["rows"], R)
        filtered = rc_cr2(w, T(c["tau"]))
        assert _same(filtered, _want_filter(w, c["tau"], T)[0])
        apart = walk(filtered, c["pos"], c["neg"], c["gate"], c["t_start"], None, np.empty((R, c["m"]), T), np.empty((R, c["m"]), T))
        want = pc.emulate_walk(filtered, c["pos"], c["neg"], c["gate"], c["t_start"], c["m"], T)
        assert np.array_equal(apart[0], want[0]) and _same(apart[1], want[1]) and _same(apart[2], want[2]), c["key"]
        found += int(apart[0].sum())
        for store_row, columns in ((True, ()), (False, ()), (False, (0, 1, 2, 3)), (True, (1, 3))):
            row, count, polarity, times = _fused(loop, w, c["tau"], c["pos"], c["neg"], c["gate"], c["t_start"], c["m"], store_row, columns)
            assert np.array_equal(count, apart[0]), (c["key"], store_row, columns, count, apart[0])
            assert _same(polarity, apart[1]) and _same(times, apart[2]), (c["key"], store_row, columns)
            assert row is None or _same(row, filtered), (c["key"], _diff(row, filtered) if row is not None else None)
    assert found > 20


def test_the_fused_walk_tests_the_value_as_stored():
    """the float32 loop's row on which the float64 state lies above a threshold and the stored float32 value on it: the walk of the state
    counts otherwise (checked first, or the case proves nothing); the fused launch gives what the two calls apart give"""
    from dspeed_amd.processors import bi_level_zero_crossing_time_points as walk
    from dspeed_amd.processors import rc_cr2

    rows, tau, pos, neg, gate, k = pc.rounding_case()
    stored, _ = _want_filter(rows, tau, np.float32)
    state, _ = pc.emulate_rc_cr2(rows, tau, np.float32, exp="libm", state=True)
    of_stored = pc.emulate_walk(stored, pos, neg, gate, 0, 5, np.float32)
    of_state = pc.emulate_walk(state, pos, neg, gate, 0, 5, np.float64)
    assert stored[0, k] == pos and state[0, k] > float(pos) and not np.array_equal(of_stored[0], of_state[0])
    filtered = rc_cr2(rows, np.float32(tau))
    assert _same(filtered, stored)
    apart = walk(filtered, pos, neg, gate, 0, None, np.empty((1, 5), np.float32), np.empty((1, 5), np.float32))
    assert np.array_equal(apart[0], of_stored[0]) and _same(apart[2], of_stored[2])
    for store_row in (True, False):
        _row, count, polarity, times = _fused("f32", rows, tau, pos, neg, gate, 0, 5, store_row, ())
        assert np.array_equal(count, of_stored[0]) and _same(times, of_stored[2]) and _same(polarity, of_stored[1]), (store_row, count, of_stored[0], of_state[0])


@pytest.mark.parametrize("rows_type", [np.float32, np.uint16, np.float64])
def test_a_subtraction_folded_into_the_launch_equals_bl_subtract_ahead_of_it(rows_type):
    """LOAD, BL_SUBTRACT, RC_CR2, BI_LEVEL_ZERO_CROSSING: one float subtraction as the rows are read -- the three gufuncs apart give the same
    bits; a NaN baseline makes its row a NaN row"""
    from dspeed_amd.processors import bi_level_zero_crossing_time_points as walk
    from dspeed_amd.processors import bl_subtract, rc_cr2

    loop = "f64" if rows_type is np.float64 else "f32"
    T = pc.LOOPS[loop]
    n, R, m = 129, 70, 5
    w = pc.tile_rows(pc.filter_rows(loop, n)[[pc.FILTER_FAMILIES.index(f) for f in ("integer", "noise", "step")]], R)
    w = (np.rint(w) + 1000).astype(rows_type)
    bl = (1000 + np.arange(R) % 7 * 0.25).astype(T)
    bl[5] = np.nan
    for baseline in (bl, 1003.5):
        sub = bl_subtract(w, baseline)
        assert _same(sub, w.astype(T) - (baseline[:, None] if isinstance(baseline, np.ndarray) else T(baseline)))
        filtered = rc_cr2(sub, 20)
        apart = walk(filtered, 40, -40, 60, 0, None, np.empty((R, m), T), np.empty((R, m), T))
        assert apart[0].sum() > 20
        for store_row in (True, False):
            row, count, polarity, times = _fused(loop, w, 20, 40, -40, 60, 0, m, store_row, (), subtract=baseline)
            assert np.array_equal(count, apart[0]) and _same(polarity, apart[1]) and _same(times, apart[2]), (rows_type, store_row)
            assert row is None or _same(row, filtered), _diff(row, filtered)
            if isinstance(baseline, np.ndarray) and row is not None:
                assert np.isnan(row[5]).all() and count[5] == 0 and np.isnan(times[5]).all()


# ---------------------------------------------------------------------------------------------------------------- 4. the fatal paths
@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_fatal_paths(loop):
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import bi_level_zero_crossing_time_points as walk
    from dspeed_amd.processors import rc_cr2

    T = pc.LOOPS[loop]
    n = 129
    w = pc.tile_rows(_quiet(loop, n), 70)
    w[67] = pc.filter_rows(loop, n)[pc.FILTER_FAMILIES.index("inf")]
    assert pc.emulate_rc_cr2(w, 20, T, exp="libm")[1].tolist() == [r == 67 for r in range(70)]
    with pytest.raises(DSPFatal, match="^RC-CR\\^2 filter produced nans in output\\.\n") as e:
        rc_cr2(w, 20)
    assert e.value.wf_range == range(67, 68)
    # the walk of the same rows does not raise: an infinite sample is an ordinary value
    lists = np.empty((70, 5), T), np.empty((70, 5), T)
    count, polarity, times = walk(w, 40, -40, 10, 0, None, *lists)
    want = pc.emulate_walk(w, 40, -40, 10, 0, 5, T)
    assert np.array_equal(count, want[0]) and _same(polarity, want[1]) and _same(times, want[2])
    # a start per event that is not integral, and one outside the row, on row 66; on a row with a NaN neither is looked at
    for bad, text in ((1.5, "The starting index must be an integer"), (float(n), "The starting index is out of range"), (-1.0, "The starting index is out of range")):
        ts = np.zeros(70, T)
        ts[66] = bad
        with pytest.raises(DSPFatal, match=f"^{text}\n") as e:
            walk(w, 40, -40, 10, ts, None, *lists)
        assert e.value.wf_range == range(66, 67)
        nan_row = [r for r in range(70) if np.isnan(w[r]).any()][0]
        ts = np.zeros(70, T)
        ts[nan_row] = bad
        count2, _p, _t = walk(w, 40, -40, 10, ts, None, *lists)
        assert np.array_equal(count2, want[0])
        with pytest.raises(DSPFatal, match=f"^{text}\n"):  # as a constant: for the whole call
            walk(w, 40, -40, 10, bad, None, *lists)
    # a gate per event that is not finite: a NaN row, count 0
    gate = np.full(70, 10, T)
    gate[[3, 5]] = np.nan, np.inf
    count3, p3, t3 = walk(w, 40, -40, gate, 0, None, *lists)
    assert count3[3] == 0 and count3[5] == 0 and np.isnan(p3[[3, 5]]).all() and np.isnan(t3[[3, 5]]).all()
    keep = [r for r in range(70) if r not in (3, 5)]
    assert np.array_equal(count3[keep], want[0][keep]) and _same(t3[keep], want[2][keep])
    for g in (np.nan, np.inf):
        with pytest.raises(ValueError, match="gate_time_in is a finite number of samples"):
            walk(w, 40, -40, g, 0, None, *lists)
    with pytest.raises(DSPFatal, match="^The length of the waveform must be larger than 3 for the filter to work safely"):
        rc_cr2(np.zeros((2, 3), T), 20)
    with pytest.raises(NotImplementedError, match="t_tau is a constant of the call on the device, not a per-event value"):
        rc_cr2(w, np.full(70, 20, T))


# ---------------------------------------------------------------------------------------------------------------- 5. the recipe
M = "dspeed.processors"
WALK = "n_crossings, polarity_out, trig_times"
LISTS = 4  # shorter than what noisy rows cross: the count goes on past them


def _tagger_rows(n_rows=70, n=1000):
    rng = np.random.default_rng(5)
    w = 1000 + rng.integers(-3, 4, (n_rows, n))  # quiet noise: below the thresholds behind the shaper
    w[:, n // 3:] += 400  # a step: the shaper's bipolar answer, one crossing
    w[::7] = 1000  # flat rows: nothing to find
    w[3::10, n // 2:] += 900  # a second step: pile-up
    w[4::10] += rng.integers(-60, 60, (len(w[4::10]), n))  # loud rows: more crossings than the lists hold
    return w.astype(np.uint16), (1000 + np.arange(n_rows) % 5).astype(np.float32)


def _tagger():
    return {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "baseline", "wf_blsub"]},
            "wf_rc": {"function": "rc_cr2", "module": f"{M}.rc_cr2", "args": ["wf_blsub", "320*ns", "wf_rc"]},
            WALK: {"function": "bi_level_zero_crossing_time_points", "module": f"{M}.time_point_thresh",
                   "args": ["wf_rc", 25, -25, 200, 0, "n_crossings", f"polarity_out({LISTS}, vector_len=n_crossings)", f"trig_times({LISTS}, vector_len=n_crossings)"]}}


def _tagger_model(w, bl):
    y = w.astype(np.float32) - bl[:, None]
    filtered, fatal = _want_filter(y, 20, np.float32)  # 320 ns on the 16 ns grid
    assert not fatal.any()
    return (filtered,) + pc.emulate_walk(filtered, 25, -25, 200, 0, LISTS, np.float32)


def test_the_pile_up_tagger_recipe_bit_for_bit():
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    w, bl = _tagger_rows()
    filtered, count, polarity, times = _tagger_model(w, bl)
    assert (count == 0).any() and (count > LISTS).any() and (count[count > 0] <= LISTS).any()  # the rows are not trivial
    for outputs in (["n_crossings", "polarity_out", "trig_times"], ["n_crossings", "polarity_out", "trig_times", "wf_rc"]):
        chain, _, out = build_processing_chain({"outputs": outputs, "processors": _tagger()}, {"waveform": WaveformInput(w, 16.0), "baseline": bl})
        chain.execute()
        assert [kernel for _what, kernel in chain.kernels()].count(pc.KERNEL) == 1 and len(chain._stages) == 1
        assert out["n_crossings"].dtype == np.uint32 and np.array_equal(out["n_crossings"], count)
        assert _same(np.asarray(out["polarity_out"]), polarity) and _same(np.asarray(out["trig_times"]), times), _diff(np.asarray(out["trig_times"]), times)
        assert "wf_rc" not in outputs or _same(np.asarray(out["wf_rc"]), filtered)


def test_build_dsp_delivers_the_lists_with_clipped_lengths():
    from lgdo_standins import Array, Table, WaveformTable

    from dspeed_amd import lgdo_io
    from dspeed_amd.build_dsp import build_dsp

    w, bl = _tagger_rows()
    _filtered, count, _polarity, times = _tagger_model(w, bl)
    res = build_dsp(Table(waveform=WaveformTable(w, 16.0, np.zeros(len(w))), baseline=Array(bl)), dsp_config={"outputs": ["n_crossings", "trig_times"], "processors": _tagger()})
    n = res["n_crossings"]
    n = np.asarray(n.nda if hasattr(n, "nda") else n)
    assert n.dtype == np.uint32 and np.array_equal(n, count)  # the count as the reference counts it
    vov = res["trig_times"]
    flat, cum = vov.to_flat() if isinstance(vov, lgdo_io.RaggedColumn) else (np.asarray(vov.flattened_data.nda), np.asarray(vov.cumulative_length.nda))
    kept = np.minimum(count, LISTS)
    assert np.array_equal(cum, np.cumsum(kept)) and np.array_equal(flat, np.concatenate([times[r, :k] for r, k in enumerate(kept)]))
