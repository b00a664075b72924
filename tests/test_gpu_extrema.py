"""get_multi_local_extrema on the device (dsp_extrema.hip) against the reference's own outputs (tests/golden/get_multi_local_extrema.npz,
what test_extrema_cases_cpu.py vouches for): bit for bit -- indices, NaN padding, counts, dtypes."""
import ctypes as C

import numpy as np
import pytest

import extrema_cases as xc
import golden_util

pytestmark = pytest.mark.gpu

WHAT = ("vt_max", "vt_min", "n_max", "n_min")


@pytest.fixture(scope="module")
def book():
    return golden_util.cases(xc.BOOK, kernel=xc.KERNEL)


def _want(c, d, m, rows=slice(None)):
    return [c[xc.key(d, m, what)][rows] for what in WHAT]


def _same(got, want, what=""):
    for g, w, name in zip(got, want, WHAT):
        g = g.to_numpy() if hasattr(g, "to_numpy") else np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w, equal_nan=True), (what, name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])


def _run(w, par, d, m, loop, counts=True):
    from dspeed_amd.processors import get_multi_local_extrema

    n_wf = len(w)
    out = [np.full((n_wf, m), -7, dtype=loop), np.full((n_wf, m), -7, dtype=loop)]
    cnt = [np.full(n_wf, 99, dtype=np.uint32), np.full(n_wf, 99, dtype=np.uint32)] if counts else []
    ret = get_multi_local_extrema(w, par[0], par[1], d, par[2], par[3], *out, *cnt)
    assert ret[0] is out[0] and ret[1] is out[1] and (not counts or (ret[2] is cnt[0] and ret[3] is cnt[1]))
    return ret


def test_every_case_of_the_book_bit_for_bit(book):
    """every group in one launch per (search_direction, m): rows of different cases side by side, each with its own four parameters as
    per-row columns; a row count that is no multiple of four among them"""
    assert any(len(c["w"]) % 4 for c in book)
    n_launches = 0
    for c in book:
        for d, m in c.params["combos"]:
            _same(_run(c["w"], c["par"], d, m, c.dtype), _want(c, d, m), (c.name, d, m))
            n_launches += 1
    assert n_launches > 200


def test_constant_parameters_views_and_device_arrays(book):
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import get_multi_local_extrema

    c = next(c for c in book if c.name == "f32_n513")
    rows = [r for r, name in enumerate(c.params["rows"]) if name.split("_rev")[0] in ("zigzag", "burst", "tie", "edges_a", "edges_b", "last_sample", "inf")]
    assert len(rows) % 4 != 0 and all(np.array_equal(c["par"][:, r], c["par"][:, rows[0]]) for r in rows)
    par = [float(v) for v in c["par"][:, rows[0]]]
    for d, m in ((0, 5), (1, 20), (3, 20), (0, 512)):
        # the parameters as constants of the launch; the rows as a strided view of a wider block
        wide = np.full((len(rows), 513 + 7), np.nan, dtype=np.float32)
        wide[:, 3:516] = c["w"][rows]
        _same(_run(wide[:, 3:516], par, d, m, np.float32), _want(c, d, m, rows), ("constants", d, m))
        # one row, one-dimensional arguments, without the counts' arrays
        got = get_multi_local_extrema(c["w"][rows[0]], *par[:2], d, *par[2:], np.empty(m, np.float32), np.empty(m, np.float32))
        _same([np.asarray(g) for g in got], [w[0] for w in _want(c, d, m, rows[:1])], ("one row", d, m))
    # rows, columns and outputs that stay on the device
    d, m = 1, 5
    dev = [DeviceArray.from_numpy(np.ascontiguousarray(c["w"]))] + [DeviceArray.from_numpy(np.ascontiguousarray(col)) for col in c["par"]]
    outs = [DeviceArray((len(c["w"]), m), np.float32), DeviceArray((len(c["w"]), m), np.float32), DeviceArray((len(c["w"]),), np.uint32),
            DeviceArray((len(c["w"]),), np.uint32)]
    get_multi_local_extrema(dev[0], dev[1], dev[2], d, dev[3], dev[4], *outs)
    _same(outs, _want(c, d, m), "device arrays")


def test_steady_state_256_rows_of_8192(book):
    c = next(c for c in book if c.name == "f32_n8192")
    reps = -(-256 // len(c["w"]))
    w = np.tile(c["w"], (reps, 1))[:256]
    par = np.tile(c["par"], (1, reps))[:, :256]
    for d, m in ((0, 20), (1, 8191), (3, 20)):
        _same(_run(w, par, d, m, np.float32), [np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:256] for a in _want(c, d, m)], ("steady", d, m))


def test_c_abi_entry_on_unaligned_strided_rows(book):
    """dsp_get_multi_local_extrema_f32 called directly: int16 rows 517 elements apart from an odd element on (the one-sample-per-lane
    kernel), a per-event column for one parameter and constants for the others, lists 24 elements apart"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray

    c = next(c for c in book if c.name == "i16_n513")
    rows = [r for r, name in enumerate(c.params["rows"]) if name in ("edges_a", "edges_b", "zigzag", "tie", "burst")]
    n_wf, n, m, d = len(rows), 513, 20, 0
    block = np.zeros(n_wf * 517 + 1, dtype=np.int16)
    for k, r in enumerate(rows):
        block[1 + k * 517: 1 + k * 517 + n] = c["w"][r]
    dblock = DeviceArray.from_numpy(block)
    col = DeviceArray.from_numpy(np.ascontiguousarray(c["par"][0, rows]))
    vt = [DeviceArray.from_numpy(np.full((n_wf, 24), -7, dtype=np.float32)) for _ in range(2)]
    cnt = [DeviceArray.from_numpy(np.full(n_wf, 99, dtype=np.uint32)) for _ in range(2)]
    row = C.c_int64(-1)
    rc = _lib.lib().dsp_get_multi_local_extrema_f32(dblock.ptr + 2, _lib.I16, n_wf, n, 517, col.ptr, 0.0, None, 5.0, d, None, -np.inf, None, np.inf, vt[0].ptr,
                                                   vt[1].ptr, m, 24, cnt[0].ptr, cnt[1].ptr, None, C.byref(row))
    assert rc == 0, _lib.last_error()
    want = _want(c, d, m, rows)
    for k in range(2):
        got = vt[k].to_numpy()
        assert np.array_equal(got[:, :m], want[k], equal_nan=True) and (got[:, m:] == -7).all()
        assert np.array_equal(cnt[k].to_numpy(), want[2 + k])


def test_the_three_fatal_texts_and_the_row_of_a_bad_delta():
    from dspeed_amd.errors import DSPFatal

    rng = np.random.default_rng(5)
    w = rng.standard_normal((9, 40)).astype(np.float32)
    par = (1.0, 1.0, -np.inf, np.inf)
    with pytest.raises(DSPFatal, match="The length of your return array must be smaller than the length of your waveform"):
        _run(w, par, 0, 40, np.float32)
    with pytest.raises(DSPFatal, match="Delta must be positive"):
        _run(w, (1.0, -0.5, -np.inf, np.inf), 0, 5, np.float32)
    with pytest.raises(DSPFatal, match="search direction type not found."):
        _run(w, par, 4, 5, np.float32)
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema"):
        _run(w, par, 2, 5, np.float32)
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema"):
        _run(np.zeros((3, 200), np.float32), par, 3, 65, np.float32)
    # a delta per event: the device's error word names the first row that got past the NaN rule with a negative one
    deltas = np.ones(9, dtype=np.float32)
    deltas[[2, 6]] = -1.0
    w[2, 7] = np.nan  # (row 2 returns NaN lists ahead of the check, as in the reference)
    with pytest.raises(DSPFatal, match="Delta must be positive") as e:
        _run(w, (deltas, 1.0, -np.inf, np.inf), 1, 5, np.float32)
    assert e.value.wf_range == range(6, 7)
    # a NaN delta is no fault: NaN lists, counts 0
    got = _run(w[:1], (np.nan, 1.0, -np.inf, np.inf), 0, 5, np.float32)
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and got[2][0] == 0 and got[3][0] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# recipes
# ------------------------------------------------------------------------------------------------------------------------------------
M = "dspeed.processors"
KEY = "vt_max_out, vt_min_out, n_max_out, n_min_out"
OUTS = ["vt_max_out", "vt_min_out", "n_max_out", "n_min_out"]


def _peaks(src, args, lists, unit):
    return {"function": "get_multi_local_extrema", "module": M, "args": [src, *args, *lists, "n_max_out", "n_min_out"], "unit": unit}


def _case(book, kind):
    return next(c for c in book if c.name == f"{kind}_n{xc.RECIPE_N}")


def test_the_reference_s_own_test_recipe_on_the_waveform_input(book):
    """tests/test_processing_chain.py:263-286 of the reference: the processor on the input rows, constants 5, 5, 0, 10, 0, lists of 10"""
    from dspeed_amd.processing_chain import build_processing_chain

    c = _case(book, "rcp")
    recipe = {"outputs": OUTS, "processors": {KEY: _peaks("waveform", [5, 5, 0, 10, 0], ["vt_max_out(10)", "vt_min_out(10)"], "ADC")}}
    chain, _, out = build_processing_chain(recipe, {"waveform": c["w"]})
    chain.execute()
    assert "dsp_extrema_kernel" in [kernel for _what, kernel in chain.kernels()]
    _same([out[o] for o in OUTS], _want(c, 0, 10), "reference recipe")
    assert (c[xc.key(0, 10, "n_max")] > 1).any() and (c[xc.key(0, 10, "n_min")] > 1).any()


def test_a_recipe_on_an_intermediate_with_thresholds_from_a_fit(book):
    """bl_subtract -> pole_zero -> the extrema of the result, backwards, with deltas and a threshold made from linear_slope_fit's outputs:
    what the reference's body returns for the oracle's pole_zero rows and the same float32 expressions of the oracle's fit"""
    from dspeed_amd.processing_chain import build_processing_chain

    c = _case(book, "rcppz")
    procs = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "baseline", "wf_blsub"]},
             "wf_pz": {"function": "pole_zero", "module": M, "args": ["wf_blsub", xc.RECIPE_TAU, "wf_pz"]},
             "bl_mean, bl_std, bl_slope, bl_intercept": {"function": "linear_slope_fit", "module": M,
                                                         "args": [f"wf_blsub[0:{xc.RECIPE_FIT}]", "bl_mean", "bl_std", "bl_slope", "bl_intercept"]},
             KEY: _peaks("wf_pz", ["5*bl_std", "bl_std", 1, "bl_mean + 3*bl_std", 0], ["vt_max_out(20)", "vt_min_out(20)"], "none")}
    chain, _, out = build_processing_chain({"outputs": OUTS + ["bl_mean", "bl_std"], "processors": procs}, {"waveform": c["raw"], "baseline": c["baseline"]})
    chain.execute()
    kernels = [kernel for _what, kernel in chain.kernels()]
    assert "dsp_extrema_kernel" in kernels and "dsp_pz_rows_kernel" in kernels
    _same([out[o] for o in OUTS], _want(c, 1, 20), "intermediate source")
    assert (c[xc.key(1, 20, "n_max")] > 1).any()


def test_computed_vector_len_leaves_build_dsp_as_a_vector_of_vectors(book):
    """vector_len = n_max_out, the lists in ns: the VectorOfVectors stand-in receives the first n_max_out times of every row, flattened, and their
    cumulative lengths; the count the recipe did not ask for stays out of the table"""
    from lgdo_standins import Table, WaveformTable

    from dspeed_amd import lgdo_io
    from dspeed_amd.build_dsp import build_dsp

    c = _case(book, "rcp")
    recipe = {"outputs": ["vt_max_out", "n_min_out"], "processors": {
        KEY: _peaks("waveform", [5, 5, 0, 10, 0], ["vt_max_out(20, vector_len=n_max_out)", "vt_min_out(20)"], ["ns", "ns", "none", "none"])}}
    n_rows = len(c["w"])
    res = build_dsp(Table(waveform=WaveformTable(c["w"], 16.0, np.zeros(n_rows))), dsp_config=recipe)
    assert "n_max_out" not in res
    vov = res["vt_max_out"]
    if isinstance(vov, lgdo_io.RaggedColumn):
        flat, cum = vov.to_flat()
    else:
        flat, cum = np.asarray(vov.flattened_data.nda), np.asarray(vov.cumulative_length.nda)
    want, counts = c[xc.key(0, 20, "vt_max")], c[xc.key(0, 20, "n_max")]
    assert np.array_equal(cum, np.cumsum(counts)) and counts.max() > 1
    assert flat.dtype == np.float32 and np.array_equal(flat, np.concatenate([want[r, :k] * np.float32(16.0) for r, k in enumerate(counts)]))
    n_min = res["n_min_out"]
    n_min = np.asarray(n_min.nda if hasattr(n_min, "nda") else n_min)
    assert n_min.dtype == np.uint32 and np.array_equal(n_min, c[xc.key(0, 20, "n_min")])


def test_recipes_that_are_refused_name_the_processor(book, monkeypatch):
    from dspeed_amd.processing_chain import build_processing_chain

    tb = {"waveform": _case(book, "rcp")["w"]}
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema"):
        build_processing_chain({"outputs": OUTS, "processors": {KEY: _peaks("waveform", [5, 5, 2, 10, 0], ["vt_max_out(10)", "vt_min_out(10)"], "ADC")}}, tb)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema"):
        build_processing_chain({"outputs": OUTS, "processors": {KEY: _peaks("waveform", [5, 5, 0, 10, 0], ["vt_max_out(10)", "vt_min_out(10)"], "ADC")}}, tb)
