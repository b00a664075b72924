"""Every compiled variant and every admission boundary of the three lane-per-waveform kernels against the CPU oracle run processor by
processor: dsp_current_kernel<SH, SCAN> (dsp_current.hip), rows_produce<IN, PZ, STOP> x rows_consume<TRAP, RPOW2, TPT, STOP>
(dsp_rows.hip) and dsp_fit_rows_kernel<T, InT> (dsp_fit.hip).  These kernels promise every output bit-identical to the oracle, so indices,
extremes, threshold time points, wavelet coefficients and the fit's mean and deviation are compared with array_equal (NaN equal to NaN);
the fit's slope and intercept -- unpinned in the oracle itself -- with the bar of test_gpu_fit_rows.  The cases, their rows and what
makes them worth running are in lane_kernel_cases.py; test_lane_kernel_cases_cpu.py checks on the oracle alone that each of them says
something.  DESIGN.md section 4c lists the variants beside the test here that runs each."""
import numpy as np
import pytest

import lane_kernel_cases as K
import oracle
from test_gpu_fit_rows import _close, _fit_rows

pytestmark = pytest.mark.gpu


def _run(recipe, tb, fused=True, promise=False):
    from dspeed_amd.processing_chain import build_processing_chain

    chain, _, out = build_processing_chain(recipe, tb)
    if promise:
        K.set_load_promise(chain.program)
        assert chain.program.ops[0][4][2] & 1  # DSP_OP_LOAD ip[2]: the rows are free of NaN or NaN throughout
    chain._ensure()
    chain._chain.set_fused(1 if fused else 0)
    chain.execute()
    return chain, out


def _same(out, want, names):
    for nm in names:
        bad = np.flatnonzero(~((out[nm] == want[nm]) | (np.isnan(out[nm]) & np.isnan(want[nm]))).reshape(len(want[nm]), -1).all(axis=1))
        assert np.array_equal(out[nm], want[nm], equal_nan=True), (nm, bad[:10], out[nm][bad[:4]], want[nm][bad[:4]])


def _vm_bar(got, want):
    """the bar of test_gpu_current_kernel for a current branch on the waveform VM (its moving averages replay the rounding): NaN where the
    oracle has NaN, elsewhere within 2e-6 of the largest value"""
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    assert np.all(np.abs(got[ok] - want[ok]) <= 2e-6 * np.abs(want[ok]).max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------------------------------
# current branch
# ------------------------------------------------------------------------------------------------------------------------------------
def _current(p, wf, start, **kw):
    chain, out = _run(K.current_recipe(p), {"wf": wf, "t_start": start}, **kw)
    return chain._chain.kernel_name, out


@pytest.mark.parametrize("p", K.CURRENT_TIGHT + K.CURRENT_SMALL, ids=K.current_id)
def test_current_branch_at_the_admission_limit_and_the_smallest_shapes(p):
    wf, t0 = K.current_rows(sum(p.values()))
    start = K.current_starts(1, t0, 1024, p["n_win"])
    kernel, out = _current(p, wf, start)
    assert kernel == "dsp_current_kernel"
    want = K.current_oracle(wf, start, p)
    _same(out, want, K.CURRENT_NAMES)
    for row, exists in K.CURRENT_SPECIAL_STARTS.items():
        assert np.isnan(out["a_hi"][row]) == (not exists), row


@pytest.mark.parametrize("p", K.CURRENT_TIGHT, ids=K.current_id)
def test_current_branch_one_sample_short_of_the_limit_runs_on_the_vm(p):
    """the last upsampled sample has no current sample behind it: the reference leaves it NaN, and with it every output.  The kernel would
    read the first checkpoint of pass 1 in its place"""
    q = K.current_refused(p)
    wf, t0 = K.current_rows(sum(q.values()))
    start = K.current_starts(1, t0, 1024, q["n_win"])
    kernel, out = _current(q, wf, start)
    assert "vm" in kernel
    want = K.current_oracle(wf, start, q)
    for nm in ("a_hi", "a_lo"):
        _vm_bar(out[nm], want[nm])


def test_current_branch_row_screen_in_two_parts():
    """rows of 2052 samples: 513 float4, the screen's second part is one float4 that every lane reads.  NaNs outside the window, which
    only the screen can see: in the last float4 of the first part, in the second part, in the last row of a full group, the first row
    of the next one and the last live row of the partial group"""
    p = K.CURRENT_DEFAULT
    n, length = 140, 2052
    wf, t0 = K.current_rows(21, n, length)
    start = K.current_starts(1, t0, length, p["n_win"])
    nan_at = {30: 2047, 31: 2048, 32: 2051, 63: 10, 64: 5, 139: 2050}
    for row, col in nan_at.items():
        assert not (start[row] <= col < start[row] + p["n_win"])
        wf[row, col] = np.nan
    kernel, out = _current(p, wf, start)
    assert kernel == "dsp_current_kernel"
    _same(out, K.current_oracle(wf, start, p), K.CURRENT_NAMES)
    assert np.isnan(out["a_hi"][list(nan_at)]).all() and not np.isnan(out["a_hi"][[29, 33, 62, 65, 138]]).any()


@pytest.mark.parametrize("p", [K.CURRENT_DEFAULT] + K.CURRENT_TIGHT, ids=K.current_id)
def test_current_branch_on_rows_with_the_promise(p):
    """wf_pz = pole_zero(waveform): all NaN or free of NaN, so the LOAD carries the promise and the kernel runs without the screen
    (SCAN = false), with every upsampling factor"""
    raw, t0 = K.current_rows(22, 100, 1024)
    raw[40, 900] = np.nan
    wf, rc = oracle.pole_zero(raw, 1716.28)
    assert rc == 0 and np.isnan(wf[40]).all()
    start = K.current_starts(1, t0, 1024, p["n_win"])
    wf[41, int(start[41]) + p["n_win"] // 2] = np.inf  # (an infinity is no NaN: the promise holds, the window's own samples make the row NaN)
    chain, out = _run(K.current_recipe(p), {"wf": wf, "t_start": start}, promise=True)
    assert chain._chain.kernel_name == "dsp_current_kernel"
    _same(out, K.current_oracle(wf, start, p), K.CURRENT_NAMES)
    assert np.isnan(out["a_hi"][[40, 41]]).all() and not np.isnan(out["a_hi"][[39, 42]]).any()


def test_current_branch_infinities_constant_and_zero_rows():
    p = K.CURRENT_TIGHT[3]  # ac = 2
    n_win, ac = p["n_win"], p["ac"]
    wf, t0 = K.current_rows(23)
    start = K.current_starts(1, t0, 1024, n_win)
    s = np.nan_to_num(start).astype(np.int64)
    wf[20, s[20]] = np.inf                                  # the window's first sample
    wf[21, s[21] + ac] = -np.inf                            # sample ac: the other operand of the first difference
    wf[22, s[22] + n_win - 1] = np.inf                      # its last sample
    wf[23, s[23] + 60] = wf[23, s[23] + 60 + ac] = np.inf   # two of one sign ac apart: inf - inf inside avg_current
    wf[24, s[24] - 1] = np.inf                              # one each side of the window: nothing changes
    wf[24, s[24] + n_win] = -np.inf
    wf[30] = 1234.5                                         # a constant and an all-zero row: every average is 0, the extremes are the
    wf[31] = 0.0                                            # first occurrence, sample 0
    kernel, out = _current(p, wf, start)
    assert kernel == "dsp_current_kernel"
    _same(out, K.current_oracle(wf, start, p), K.CURRENT_NAMES)
    assert np.isnan(out["a_hi"][[20, 21, 22, 23]]).all() and np.isfinite(out["a_hi"][24])
    for nm in K.CURRENT_NAMES:
        assert np.array_equal(out[nm][[30, 31]], [0.0, 0.0]), nm


@pytest.mark.parametrize("factor", K.CURRENT_SCALES)
def test_current_branch_denormals_and_overflow(factor):
    p = K.CURRENT_DEFAULT
    wf, t0 = K.current_rows(sum(p.values()))
    wf = K.scaled(wf, factor)
    start = K.current_starts(1, t0, 1024, p["n_win"], special=False)
    kernel, out = _current(p, wf, start)
    assert kernel == "dsp_current_kernel"
    _same(out, K.current_oracle(wf, start, p), K.CURRENT_NAMES)


@pytest.mark.parametrize("where", ["first", "last"])
def test_current_branch_constant_start(where):
    p = K.CURRENT_DEFAULT
    wf, _ = K.current_rows(24)
    at = 0 if where == "first" else 1024 - p["n_win"]
    chain, out = _run(K.current_recipe(p, start=str(at)), {"wf": wf})
    assert chain._chain.kernel_name == "dsp_current_kernel"
    want = K.current_oracle(wf, np.float32(at), p)
    _same(out, want, K.CURRENT_NAMES)
    assert not np.isnan(out["a_hi"]).any()


@pytest.mark.parametrize("outputs", [("a_lo", "t_hi"), ("t_hi", "a_lo"), ("t_lo",)])
def test_current_branch_subsets_of_outputs(outputs):
    p = K.CURRENT_SMALL[1]
    wf, t0 = K.current_rows(25)
    start = K.current_starts(1, t0, 1024, p["n_win"])
    chain, out = _run(K.current_recipe(p, outputs=outputs), {"wf": wf, "t_start": start})
    assert chain._chain.kernel_name == "dsp_current_kernel" and sorted(out) == sorted(outputs)
    _same(out, K.current_oracle(wf, start, p), outputs)


# ------------------------------------------------------------------------------------------------------------------------------------
# rows kernel
# ------------------------------------------------------------------------------------------------------------------------------------
def _rows_names(c):
    return (*K.MM_NAMES, "tp_0") + (("dwt",) if c["dwt"] else ())


@pytest.mark.parametrize("c", K.ROWS_CASES + K.ROWS_HAAR + K.ROWS_INT16 + K.ROWS_SCALED, ids=lambda c: c["name"])
def test_rows_kernel_producers_levels_operands_and_magnitudes(c):
    recipe, tb, want = K.rows_case(c)
    chain, out = _run(recipe, tb)
    assert chain._chain.kernel_name == "dsp_rows_kernel"
    _same(out, want, _rows_names(c))


@pytest.mark.parametrize("n", [1, 64, 67])
@pytest.mark.parametrize("c", K.ROWS_SHORT, ids=lambda c: c["name"])
def test_rows_kernel_short_rows(c, n):
    recipe, tb, want = K.rows_case(c)  # (rows are independent: the first n of the case's 70)
    chain, out = _run(recipe, {k: v[:n] for k, v in tb.items()})
    assert chain._chain.kernel_name == "dsp_rows_kernel"
    _same(out, {k: v[:n] for k, v in want.items()}, _rows_names(c))


@pytest.mark.parametrize("c", K.ROWS_RING, ids=lambda c: c["name"])
def test_rows_kernel_ring_limit(c):
    recipe, tb, want = K.rows_case(c)
    chain, out = _run(recipe, tb)
    if c["kernel"] == "dsp_rows_kernel":
        assert chain._chain.kernel_name == "dsp_rows_kernel"
        _same(out, want, _rows_names(c))
    else:  # one sample more of lag: the waveform VM, to its own bar (rounding replay of the trapezoid): 1e-6 of the peak
        assert chain._chain.kernel_name.startswith("dsp_vm")
        peak = np.maximum(np.abs(want["wf_max"]), np.abs(want["wf_min"]))
        for nm in ("wf_max", "wf_min"):
            assert np.max(np.abs(out[nm] - want[nm]) / peak) <= 1e-6, nm


def test_rows_kernel_nan_walk_parameter():
    wf, _ = K.synth_rows(801)
    thr = K.thresholds(802)
    chain, out = _run(K.rows_recipe(K.DPZ, K.T0_TRAP, tpt=("thr", "tp_max", "np.nan")), {"waveform": wf, "thr": thr})
    assert chain._chain.kernel_name == "dsp_rows_kernel"
    want = K.rows_oracle(wf, K.DPZ, K.T0_TRAP, thr=thr, walk=np.nan)
    _same(out, want, (*K.MM_NAMES, "tp_0"))
    assert np.isnan(out["tp_0"]).all() and not np.isnan(out["wf_max"]).any()


@pytest.mark.parametrize("walk", list(K.ROWS_WALKS))
@pytest.mark.parametrize("trap", K.ROWS_TRAPS, ids=lambda t: "-".join(map(str, t)))
def test_rows_kernel_every_consumer(trap, walk):
    """rows_consume<TRAP, RPOW2, TPT>: each trapezoid, dividing by its rise or multiplying, with each of the five walks"""
    recipe, tb, want = K.walk_case(trap, walk)
    chain, out = _run(recipe, tb)
    assert chain._chain.kernel_name == "dsp_rows_kernel"
    _same(out, want, sorted(want))


@pytest.mark.parametrize("dtype,trap", K.STOP_CASES, ids=lambda v: np.dtype(v).name if isinstance(v, type) else "-".join(map(str, v)))
def test_rows_kernel_stop_build(dtype, trap):
    """the group stops behind the latest start among its 64 rows; what lies behind cannot change a walk backward"""
    recipe, tb, tp0 = K.stop_case(dtype, trap)
    chain, out = _run(recipe, tb, promise=True)
    assert chain._chain.kernel_name == "dsp_rows_kernel" and sorted(out) == ["tp_0"]
    _same(out, {"tp_0": tp0}, ("tp_0",))


# ------------------------------------------------------------------------------------------------------------------------------------
# fit kernel
# ------------------------------------------------------------------------------------------------------------------------------------
def _fit_check(got, want, fits, factor=1.0):
    for k, f in enumerate(fits):
        assert np.array_equal(got[k, 0], want[k, 0], equal_nan=True) and np.array_equal(got[k, 1], want[k, 1], equal_nan=True), f
        _close(got[k, 2], want[k, 2], K.FIT_SLOPE_SCALE * factor, f)
        _close(got[k, 3], want[k, 3], K.FIT_INTERCEPT_SCALE * factor, f)


def _aligned(w):
    """the rows in a buffer whose base and row stride are multiples of 16 bytes: the kernel's 16-byte loads"""
    pad = np.zeros((w.shape[0], (w.shape[1] + 15) // 16 * 16), dtype=w.dtype)
    pad[:, :w.shape[1]] = w
    return pad


@pytest.mark.parametrize("layout", ["stride1001", "base+1"])
@pytest.mark.parametrize("dtype,ft", K.FIT_TYPES, ids=lambda t: np.dtype(t).name)
def test_fit_rows_types_and_unaligned_rows(dtype, ft, layout):
    """two full blocks of 64 rows and a partial one; a row stride or a base that is no multiple of 16 bytes sends the full blocks down
    the element-wise staging path too: the same fits, bit for bit, as on an aligned copy of the rows"""
    n = 130
    bl = np.random.default_rng(6).uniform(2900, 3100, n).astype(np.float32)
    if layout == "stride1001":
        w = K.fit_rows(n, 1001, dtype, 31)
        fits = [(0, 0, 300), (1, 400, 601), (0, 100, 50), (1, 0, 1001)]
        got, view = _fit_rows(w, fits, bl, 1, K.FIT_TAU, ft), w
    else:
        w = K.fit_rows(n, 1000, dtype, 32)
        fits = [(0, 0, 300), (1, 400, 599), (0, 100, 50), (1, 0, 999)]
        got, view = _fit_rows(w, fits, bl, 1, K.FIT_TAU, ft, lo=1, length=999), w[:, 1:]
    assert got.dtype == ft
    same = _fit_rows(_aligned(view), fits, bl, 1, K.FIT_TAU, ft, length=view.shape[1])
    assert np.array_equal(got, same, equal_nan=True)
    _fit_check(got, K.fit_oracle(view, fits, bl.astype(ft), 1, K.FIT_TAU, ft), fits)


@pytest.mark.parametrize("dtype,ft", K.FIT_TYPES_F64_16BIT, ids=lambda t: np.dtype(t).name)
def test_fit_rows_16_bit_rows_in_the_float64_loop(dtype, ft):
    w = K.fit_rows(70, 200, dtype, 36)
    fits = [(0, 0, 64), (1, 100, 100)]
    got = _fit_rows(w, fits, 3000.0, 1, K.FIT_TAU, ft)
    assert got.dtype == ft
    _fit_check(got, K.fit_oracle(w, fits, 3000.0, 1, K.FIT_TAU, ft), fits)


def test_fit_rows_windows_at_tile_edges():
    n = 70
    w = K.fit_rows(n, 256, np.int16, 33)
    bl = np.full(n, 3000, np.float32)
    for fits in (K.FIT_TILE_EDGE_WINDOWS[:4], K.FIT_TILE_EDGE_WINDOWS[4:]):
        got = _fit_rows(w, fits, bl, 1, K.FIT_TAU)
        _fit_check(got, K.fit_oracle(w, fits, bl, 1, K.FIT_TAU, np.float32), fits)


def test_fit_rows_production_shape():
    """a stage-0 window at the start, 400 samples with no fit active (the pole-zero state carried), a stage-1 window: alone, and in slots 2
    and 3 of four"""
    n = 130
    w = K.fit_rows(n, 1000, np.int16, 34)
    bl = np.random.default_rng(7).uniform(2900, 3100, n).astype(np.float32)
    two = K.FIT_PRODUCTION_WINDOWS
    got = _fit_rows(w, two, bl, 1, K.FIT_TAU)
    _fit_check(got, K.fit_oracle(w, two, bl, 1, K.FIT_TAU, np.float32), two)
    four = [(0, 320, 40), (1, 400, 100)] + two
    got4 = _fit_rows(w, four, bl, 1, K.FIT_TAU)
    assert np.array_equal(got4[2:], got, equal_nan=True)
    _fit_check(got4, K.fit_oracle(w, four, bl, 1, K.FIT_TAU, np.float32), four)


def test_fit_rows_windows_of_one_and_two_samples():
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray, dtype_code, sync

    n = 70
    w = K.fit_rows(n, 100, np.float32, 35)
    d_w = DeviceArray.from_numpy(w)
    out = DeviceArray.from_numpy(np.full((8, n), -7.0, np.float32))
    for fits in ([(0, 10, 1)], [(0, 10, 20), (0, 99, 1)]):
        win = (_lib.FitWindow * len(fits))(*[_lib.FitWindow(*f) for f in fits])
        rc = _lib.lib().dsp_linear_slope_fit_rows(d_w.ptr, dtype_code(w.dtype), n, 100, 100, dtype_code(np.float32), None, 0, 0.0, 0, 0, 0.0,
                                                  win, len(fits), out.ptr, None)
        assert rc == _lib.E_ZERODIV and _lib.last_error() == _lib.fatal_message(_lib.E_ZERODIV)
        with pytest.raises(ZeroDivisionError):
            _lib.check(rc, what="fit rows")
        sync()
        assert np.all(out.to_numpy() == -7.0)  # nothing was launched
    fits = [(0, 10, 2), (0, 63, 2)]
    _fit_check(_fit_rows(w, fits), K.fit_oracle(w, fits, None, 0, None, np.float32), fits)
