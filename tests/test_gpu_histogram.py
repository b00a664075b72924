"""histogram and histogram_stats on the device (dsp_hist.hip) against tests/golden/histogram.npz (what test_histogram_cases_cpu.py vouches
for): weights, borders, mode, max and fwhm bit for bit -- through the gufuncs, the C entries, and programs that fuse the two."""
import ctypes as C

import numpy as np
import pytest

import golden_util
import histogram_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def book():
    return golden_util.cases(hc.BOOK, kernel=hc.KERNEL)


@pytest.fixture(scope="module")
def stats_book():
    return golden_util.cases(hc.BOOK, kernel=hc.KERNEL_STATS)


def _rows(c, m):
    x = c[hc.key(m, "x")]
    return np.concatenate([c["w"], x]) if len(x) else c["w"]


def _same(got, want, what=""):
    got = got.to_numpy() if hasattr(got, "to_numpy") else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (what, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])


def _run_program(p, loop, bufs, n_wf):
    """one launch of a program on device copies of ``bufs`` (outputs pre-filled with -7); returns the outputs"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray, sync

    ch = Chain(p, "histogram test", loop)
    assert ch.kernel_name == "dsp_hist_kernel"
    dev = {}
    for name, kind, code, length, offset, stride in p.io:
        if name in bufs:
            dev[name] = DeviceArray.from_numpy(np.ascontiguousarray(bufs[name]))
        else:
            dev[name] = DeviceArray.from_numpy(np.full((n_wf, length) if length > 1 or name in ("weights", "borders") else (n_wf,), -7, dtype=loop))
    ch.execute(dev, n_wf)
    sync()
    ch.check()
    return {name: d.to_numpy() for name, d in dev.items() if name not in bufs}


def test_every_case_of_the_book_through_the_gufunc(book):
    from dspeed_amd.processors import histogram

    assert any(len(_rows(c, m)) % 4 for c in book for m in c.params["ms"])  # a partial workgroup among the launches
    n_launches = 0
    for c in book:
        for m in c.params["ms"]:
            rows = _rows(c, m)
            wts, brd = np.full((len(rows), m), -7, dtype=c.dtype), np.full((len(rows), m + 1), -7, dtype=c.dtype)
            ret = histogram(rows, wts, brd)
            assert ret[0] is wts and ret[1] is brd
            _same(wts, c[hc.key(m, "weights")], (c.name, m, "weights"))
            _same(brd, c[hc.key(m, "borders")], (c.name, m, "borders"))
            n_launches += 1
    assert n_launches > 50  # (every group with every number of bins it is run with)


def test_every_stats_case_through_the_gufunc(stats_book):
    from dspeed_amd.processors import histogram_stats

    for c in stats_book:
        n_wf = len(c["weights"])
        outs = [np.full(n_wf, -7, dtype=c.dtype) for _ in range(3)]
        ret = histogram_stats(c["weights"], c["edges"], *outs, c["max_in"])
        assert all(r is o for r, o in zip(ret, outs))
        _same(np.stack(outs, axis=1), c["stats"], c.name)
        # one row, a constant max_in, outputs allocated
        r = n_wf // 2
        got = histogram_stats(c["weights"][r], c["edges"][r], None, None, None, c["max_in"][r])
        _same(np.array(got, dtype=c.dtype), c["stats"][r], (c.name, "one row"))


@pytest.mark.parametrize("n_wf", [1, 5])
def test_one_row_and_a_partial_workgroup(book, n_wf):
    from dspeed_amd.processors import histogram

    c = next(c for c in book if c.name == "f32_n1000")
    m = 100
    rows = _rows(c, m)[:n_wf]
    wts, brd = histogram(rows, np.empty((n_wf, m), np.float32), np.empty((n_wf, m + 1), np.float32))
    _same(wts, c[hc.key(m, "weights")][:n_wf])
    _same(brd, c[hc.key(m, "borders")][:n_wf])
    if n_wf == 1:  # one-dimensional arguments
        wts, brd = histogram(rows[0], np.empty(m, np.float32), np.empty(m + 1, np.float32))
        _same(wts, c[hc.key(m, "weights")][0])
        _same(brd, c[hc.key(m, "borders")][0])


def test_wavefronts_that_take_several_rows_zero_their_counters(book):
    """256 rows of 8192 samples dealt to 8 workgroups (the program's cap, DSP_OP_HISTOGRAM ip[1]): every wavefront takes 8 rows, each on
    counters its last row has filled"""
    c = next(c for c in book if c.name == "f32_n8192")
    m = 100
    rows = _rows(c, m)
    reps = -(-256 // len(rows))
    w = np.tile(rows, (reps, 1))[:256]
    got = _run_program(hc.hist_program(8192, m, stats=True, max_blocks=8), np.float32, {"wf": w}, 256)
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:256]  # noqa: E731
    _same(got["weights"], tile(c[hc.key(m, "weights")]), "weights")
    _same(got["borders"], tile(c[hc.key(m, "borders")]), "borders")
    _same(np.stack([got["mode"], got["max"], got["fwhm"]], axis=1), tile(c[hc.key(m, "stats")]), "stats")


def test_fused_and_unfused_agree_and_the_fused_launch_may_store_no_rows(book):
    from dspeed_amd.processors import histogram, histogram_stats

    for name, m in (("f32_n1024", 2048), ("f32_n1024", 65), ("i16_n1000", 100), ("i16_n4096", 100), ("u16_n65", 64), ("f64_n1000", 65), ("f32_n3", 1)):
        c = next(c for c in book if c.name == name)
        rows, n = _rows(c, m), c.params["n"]
        rd = np.dtype(c.params["rows_dtype"])
        wts, brd = histogram(rows, np.empty((len(rows), m), c.dtype), np.empty((len(rows), m + 1), c.dtype))
        unfused = np.stack(histogram_stats(wts, brd, None, None, None, np.nan), axis=1)
        _same(unfused, c[hc.key(m, "stats")], (name, m, "unfused"))
        for stores in (True, False):
            got = _run_program(hc.hist_program(n, m, rd, c.dtype, stats=True, stores=stores), c.dtype, {"wf": rows}, len(rows))
            _same(np.stack([got["mode"], got["max"], got["fwhm"]], axis=1), unfused, (name, m, stores))
            assert ("weights" in got) == stores
            if stores:
                _same(got["weights"], wts)
                _same(got["borders"], brd)
    # max_in per event in the fused launch: against histogram_stats alone on the same histograms
    c = next(c for c in book if c.name == "f32_n1000")
    m = 63
    rows = _rows(c, m)
    brd = c[hc.key(m, "borders")]
    max_in = np.where(np.isnan(brd[:, 0]), 1.0, brd[:, 0] + np.float32(0.4) * (brd[:, -1] - brd[:, 0])).astype(np.float32)
    max_in[::3] = np.nan
    got = _run_program(hc.hist_program(1000, m, stats=True, stores=False, max_in="column"), np.float32, {"wf": rows, "max_in": max_in}, len(rows))
    want = np.stack(histogram_stats(c[hc.key(m, "weights")], brd, None, None, None, max_in), axis=1)
    _same(np.stack([got["mode"], got["max"], got["fwhm"]], axis=1), want, "max_in column")
    want_model = np.array([hc.model_stats(c[hc.key(m, "weights")][r], brd[r], max_in[r], np.float32) for r in range(len(rows))], dtype=np.float32)
    _same(want, want_model, "model")


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("n,m", [(1023, 4), (1024, 64), (8192, 64)])
def test_a_bin_index_that_reaches_m_is_dropped_on_the_device(T, n, m):
    """rows whose largest samples below the maximum have k = m (no fixture holds one), beside ordinary rows in the same workgroups: a sample
    per lane (1023) and whole vectors, a row in registers and a row read twice; with 64 bins counter 64 is the next wavefront's first.  The
    dropped samples are counted nowhere, and the rows beside them are what they are alone."""
    from dspeed_amd.processors import histogram

    rows, want, dropped = hc.dropping_rows(n, m, T)
    assert dropped[[1, 2, 4]].min() > 0 and not dropped[[0, 3, 5]].any()
    wts, brd = histogram(rows, np.full((6, m), -7, dtype=T), np.full((6, m + 1), -7, dtype=T))
    _same(wts, want, (n, m, "weights"))
    model = [hc.model_histogram(rows[r], m, T, 1) for r in range(6)]
    _same(wts, np.array([w for w, _ in model]), "model weights")
    _same(brd, np.array([b for _, b in model]), "model borders")
    assert np.array_equal((rows != rows.max(axis=1, keepdims=True)).sum(axis=1) - wts.sum(axis=1).astype(np.int64), dropped)
    for r in (0, 3, 5):  # the ordinary rows, each alone
        alone = histogram(rows[r:r + 1], np.empty((1, m), T), np.empty((1, m + 1), T))
        _same(alone[0][0], wts[r])
        _same(alone[1][0], brd[r])


def test_c_abi_entries_on_unaligned_strided_rows(book, stats_book):
    """dsp_histogram_f32 called directly: int16 rows 1003 elements apart from an odd element on (the one-sample-per-lane kernel), weights 104
    and borders 103 elements apart; dsp_histogram_stats_f32 on those rows as they lie, with a max_in column"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray

    c = next(c for c in book if c.name == "i16_n1000")
    n, m = 1000, 100
    rows = _rows(c, m)
    n_wf = len(rows)
    block = np.zeros(n_wf * 1003 + 1, dtype=np.int16)
    for k in range(n_wf):
        block[1 + k * 1003: 1 + k * 1003 + n] = rows[k]
    dblock = DeviceArray.from_numpy(block)
    wts = DeviceArray.from_numpy(np.full((n_wf, 104), -7, dtype=np.float32))
    brd = DeviceArray.from_numpy(np.full((n_wf, 103), -7, dtype=np.float32))
    row = C.c_int64(-1)
    rc = _lib.lib().dsp_histogram_f32(dblock.ptr + 2, _lib.I16, n_wf, n, 1003, wts.ptr, m, 104, brd.ptr, m + 1, 103, None, C.byref(row))
    assert rc == 0, _lib.last_error()
    _same(wts.to_numpy()[:, :m], c[hc.key(m, "weights")])
    _same(brd.to_numpy()[:, :m + 1], c[hc.key(m, "borders")])
    assert (wts.to_numpy()[:, m:] == -7).all() and (brd.to_numpy()[:, m + 1:] == -7).all()
    outs = [DeviceArray.from_numpy(np.full(n_wf, -7, dtype=np.float32)) for _ in range(3)]
    col = DeviceArray.from_numpy(np.full(n_wf, np.nan, dtype=np.float32))
    rc = _lib.lib().dsp_histogram_stats_f32(wts.ptr, n_wf, m, 104, brd.ptr, m + 1, 103, col.ptr, 0.0, outs[0].ptr, outs[1].ptr, outs[2].ptr, None, C.byref(row))
    assert rc == 0, _lib.last_error()
    _same(np.stack([o.to_numpy() for o in outs], axis=1), c[hc.key(m, "stats")])
    # the float64 entry on aligned rows
    c = next(c for c in book if c.name == "f64_n257")
    m = 64
    rows = np.ascontiguousarray(_rows(c, m))
    d = DeviceArray.from_numpy(rows)
    wts, brd = DeviceArray((len(rows), m), np.float64), DeviceArray((len(rows), m + 1), np.float64)
    rc = _lib.lib().dsp_histogram_f64(d.ptr, _lib.F64, len(rows), 257, 257, wts.ptr, m, m, brd.ptr, m + 1, m + 1, None, C.byref(row))
    assert rc == 0, _lib.last_error()
    _same(wts, c[hc.key(m, "weights")])
    _same(brd, c[hc.key(m, "borders")])


def test_an_infinite_sample_makes_a_nan_row_and_the_reference_checks_hold():
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import histogram, histogram_stats

    w = np.arange(40, dtype=np.float32).reshape(4, 10)
    w[1, 3], w[2, 9] = np.inf, -np.inf
    wts, brd = histogram(w, np.empty((4, 5), np.float32), np.empty((4, 6), np.float32))
    assert not wts[1:3].any() and np.isnan(brd[1:3]).all() and wts[0].sum() == 9 and wts[3].sum() == 9
    with pytest.raises(DSPFatal, match="length borders_out must be exactly 1 \\+ length of weights_out"):
        histogram(w, np.empty((4, 5), np.float32), np.empty((4, 5), np.float32))
    with pytest.raises(DSPFatal, match="length edges_in must be exactly 1 \\+ length of weights_in"):
        histogram_stats(wts, np.ascontiguousarray(brd[:, :5]), None, None, None, np.nan)
    with pytest.raises(NotImplementedError, match="at most 2048 bins"):
        histogram(w, np.empty((4, 2049), np.float32), np.empty((4, 2050), np.float32))
    with pytest.raises(NotImplementedError, match="float64 loop takes float64 rows"):
        histogram(w.astype(np.int32), np.empty((4, 5), np.float64), np.empty((4, 6), np.float64))


def test_the_sipm_fragment_as_a_recipe_with_the_reference_s_module_strings():
    """avg_current -> histogram -> histogram_stats -> get_multi_local_extrema with 3*fwhm through build_processing_chain, against the models of
    the two kernels chained on the CPU (each held against the reference's bodies by its own CPU test): lists, counts, fwhm bit for bit"""
    import extrema_cases as xc

    from dspeed_amd.processing_chain import build_processing_chain

    w = hc.sipm_rows()
    outs = ["vt_max_candidate_out", "vt_min_out", "n_max_out", "n_min_out", "fwhm", "idx_out_c", "max_out"]
    chain, _, out = build_processing_chain({"outputs": outs, "processors": hc.sipm_fragment()}, {"waveform": w})
    chain.execute()
    kernels = [kernel for _what, kernel in chain.kernels()]
    assert kernels.count("dsp_hist_kernel") == 1 and "dsp_extrema_kernel" in kernels
    x = w.astype(np.float32)
    curr = ((x[:, 5:] - x[:, :-5]) / np.float32(5)).astype(np.float32)
    want = {k: [] for k in outs}
    for row in curr:
        wts, brd = hc.model_histogram(row, 100, np.float32, 1)
        mode, edge, fwhm = hc.model_stats(wts, brd, np.nan, np.float32)
        lists = xc.model(row, 5, 0.1, 1, np.float32(3) * fwhm, 0, 20, np.float32, 1)
        for k, v in zip(outs, (*lists, fwhm, mode, edge)):
            want[k].append(v)
    for k in outs:
        _same(out[k], np.array(want[k], dtype=np.uint32 if k.startswith("n_") else np.float32), k)
    counts = np.array(want["n_max_out"])
    assert counts.min() == 0 and counts.max() > 1 and np.isfinite(np.array(want["fwhm"])).all()
    # the threshold matters: without it the noise's own maxima fill the lists
    free = [int(xc.model(row, 5, 0.1, 1, -np.inf, 0, 20, np.float32, 1)[2]) for row in curr]
    assert sum(free) > counts.sum()
