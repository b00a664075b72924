"""log_check, poly_fit, poly_diff and poly_exp_rms on the device (dsp_tailfit.hip): the whole book of tests/tailfit_cases.py against its
emulation, both loops -- poly_fit, poly_diff and log_check's NaN pattern bit for bit, log_check's values and poly_exp_rms within the bounds
the case module derives (the device's log and exp are not NumPy's) --, through the gufuncs and, for the layouts a gufunc call cannot make
(padded strides, a non-zero start, a sentinel behind every output, int16 and uint16 rows), through the C entries; the fused launches
against the calls apart; the docstring recipe.  Wherever a fit follows a logarithm the yardstick is fed the logged row the device stored,
so that the fit is compared bit for bit whatever the last bit of a logarithm."""
import os

import numpy as np
import pytest

import tailfit_cases as tc

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
CODES = {np.dtype(np.float32): "F32", np.dtype(np.int16): "I16", np.dtype(np.uint16): "U16", np.dtype(np.float64): "F64"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{tc.BOOK}.npz")


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return int(bad.sum()), [i[:6].tolist() for i in np.nonzero(bad)], got[bad][:4], want[bad][:4]


def _log_ok(got, rows, T, what):
    """the NaN pattern exactly, the values within the bound"""
    want = tc.emulate_log_check(rows, T)
    assert got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)), what
    exact, bound = tc.log_bound(rows, T)
    ok, ratio = tc.within(got, exact, bound, want)
    assert ok, (what, ratio)
    return ratio


def _exp_ok(mean, rms, rows, pars, T, what):
    want = tc.emulate_residual(rows, pars, T, True)
    x_mean, x_rms, b_mean, b_rms = tc.residual_bound(rows, pars, T, True)
    ok_m, r_m = tc.within(mean, x_mean, b_mean, want[0])
    ok_r, r_r = tc.within(rms, x_rms, b_rms, want[1])
    assert ok_m and ok_r, (what, r_m, r_r)
    return max(r_m, r_r)


# ---------------------------------------------------------------------------------------------------------------- 1. the whole book
@pytest.mark.parametrize("loop", list(tc.LOOPS))
def test_the_book_through_the_gufuncs(loop):
    from dspeed_amd.processors import log_check, poly_diff, poly_exp_rms, poly_fit

    T = tc.LOOPS[loop]
    book = np.load(GOLDEN)
    worst = [0.0, 0.0]
    for index, n in enumerate(tc.LENGTHS):
        R = tc.ROW_COUNTS[index % len(tc.ROW_COUNTS)]
        w = tc.tile_rows(tc.tail_rows(loop, n), R)
        before = w.copy()
        out = np.full((R, n), SENTINEL, T)
        assert log_check(w, out) is out
        worst[0] = max(worst[0], _log_ok(out, w, T, (n, R)))
        assert w.tobytes() == before.tobytes()
    index = 0
    for n, m in tc.fit_cases():
        fitter = poly_fit(n, m - 1)
        assert fitter.__name__ == "poly_fitter" and np.array_equal(fitter.inv, tc.inverse(n, m - 1))
        for rows in (tc.tail_rows(loop, n), tc.emulate_log_check(tc.tail_rows(loop, n), T)):
            index += 1
            R = tc.ROW_COUNTS[index % len(tc.ROW_COUNTS)]
            w = tc.tile_rows(rows, R)
            pars = np.full((R, m), SENTINEL, T)
            assert fitter(w, pars) is pars
            want = tc.emulate_poly_fit(w, fitter.inv, T)
            assert tc.same(pars, want), (n, m, R, _diff(pars, want))
    for n in tc.LENGTHS:
        for m in tc.MS:
            index += 1
            R = tc.ROW_COUNTS[index % len(tc.ROW_COUNTS)]
            rows, pars = tc.residual_case(loop, n, m)
            w, p = tc.tile_rows(rows, R), tc.tile_rows(pars, R)
            mean, rms = poly_diff(w, p)
            want = tc.emulate_residual(w, p, T, False)
            assert tc.same(mean, want[0]) and tc.same(rms, want[1]), (n, m, R, _diff(mean, want[0]), _diff(rms, want[1]))
            if loop == "f64":  # the float64 loop against the reference's own run
                full = poly_diff(rows, pars)
                assert tc.same(full[0], book[f"diff_f64_n{n}_m{m}/mean"]) and tc.same(full[1], book[f"diff_f64_n{n}_m{m}/rms"]), (n, m)
            mean, rms = np.full(R, SENTINEL, T), np.full(R, SENTINEL, T)
            got = poly_exp_rms(w, p, mean, rms)
            assert got[0] is mean and got[1] is rms
            worst[1] = max(worst[1], _exp_ok(mean, rms, w, p, T, (n, m, R)))
    print(f"{loop}: worst |got - exact| / bound: log_check {worst[0]:.3g}, poly_exp_rms {worst[1]:.3g}")
    # 1-D calls, one set of coefficients for every row
    row, p = tc.tail_rows(loop, 129)[0], tc.coefficients(loop, 4, 129)[0]
    assert log_check(row).shape == (129,) and poly_fit(129, 3)(row).shape == (4,)
    mean, rms = poly_diff(row, p)
    want = tc.emulate_residual(row, p, T, False)
    assert np.ndim(mean) == 0 and tc.same(np.asarray(mean)[None], want[0]) and tc.same(np.asarray(rms)[None], want[1])
    w = tc.tail_rows(loop, 65)
    assert tc.same(poly_diff(w, p)[1], tc.emulate_residual(w, np.broadcast_to(p, (len(w), 4)), T, False)[1])


# ---------------------------------------------------------------------------------------------------------------- 2. the C entries
def _blocks(w, in_off, in_stride):
    block = np.full(8 + len(w) * in_stride, 77, dtype=w.dtype)
    block[in_off:in_off + len(w) * in_stride].reshape(len(w), in_stride)[:, :w.shape[1]] = w
    return block


def _rows_out(dev, off, R, stride, width):
    """(the rows written, is everything around them untouched)"""
    got = dev.to_numpy()
    body = got[off:off + R * stride].reshape(R, stride)
    return np.ascontiguousarray(body[:, :width]), bool((got[:off] == SENTINEL).all() and (body[:, width:] == SENTINEL).all() and (got[off + R * stride:] == SENTINEL).all())


@pytest.mark.parametrize("rows_type", [np.float32, np.int16, np.uint16, np.float64])
def test_layouts_through_the_c_entries_with_sentinels(rows_type):
    """rows n or n + 3 apart, from a 16-byte boundary or from an element 1 .. 3 past one (a slice with a non-zero start), outputs likewise:
    16-byte loads and stores where start and stride allow, an element per lane otherwise, and nothing but the outputs written"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.gufunc import run

    L = _lib.lib()
    loop = "f64" if rows_type is np.float64 else "f32"
    T = tc.LOOPS[loop]
    esz, isz = np.dtype(T).itemsize, np.dtype(rows_type).itemsize
    loop_code, code = _lib.F32 if T is np.float32 else _lib.F64, getattr(_lib, CODES[np.dtype(rows_type)])
    integer = np.dtype(rows_type).kind in "iu"
    vectors = set()
    for index, n in enumerate(tc.LENGTHS + (512,)):
        base = tc.tail_rows(loop, n)
        if integer:  # whole numbers in the type's range; a NaN or an infinity has no integer: those rows become rows of 7
            base = np.where(np.isfinite(base), np.rint(base), 7)
            base = np.abs(base) if rows_type is np.uint16 else base
        R = tc.ROW_COUNTS[index % len(tc.ROW_COUNTS)]
        w = tc.tile_rows(base, R).astype(rows_type)
        for padded in (False, True):
            in_off, in_stride = (1 + index % 3, n + 3) if padded else (0, n)
            off, out_stride = ((index // 2) % 4, n + 3) if padded else (0, n)
            vectors.add((in_off * isz % 16 == 0 and in_stride * isz % 16 == 0 and n * isz % 16 == 0, off * esz % 16 == 0 and out_stride * esz % 16 == 0))
            block = _blocks(w, in_off, in_stride)
            d = DeviceArray.from_numpy(block)
            rows_args = (d.ptr + in_off * isz, code, R, n, in_stride, loop_code)
            # log_check
            o = DeviceArray.from_numpy(np.full(4 + R * out_stride + 8, SENTINEL, T))
            run(L.dsp_log_check_rows, "log_check", *rows_args, o.ptr + off * esz, out_stride)
            got, clean = _rows_out(o, off, R, out_stride, n)
            _log_ok(got, w, T, (rows_type, n, padded))
            assert clean, (rows_type, n, padded)
            o.free()
            # poly_fitter
            for m in (mm for mm in tc.MS if mm <= n and (mm == tc.MS[index % 4] or n == 129)):
                inv = tc.inverse(n, m - 1)
                dinv = DeviceArray.from_numpy(np.ascontiguousarray(inv))
                p_stride = m + 3 if padded else m
                o = DeviceArray.from_numpy(np.full(4 + R * p_stride + 8, SENTINEL, T))
                run(L.dsp_poly_fit_rows, "poly_fit", *rows_args, dinv.ptr, m, o.ptr + off * esz, p_stride)
                got, clean = _rows_out(o, off, R, p_stride, m)
                want = tc.emulate_poly_fit(w, inv, T)
                assert tc.same(got, want) and clean, (rows_type, n, m, padded, _diff(got, want))
                o.free(), dinv.free()
            # the residuals: coefficients a row per event, m or m + 3 apart
            for m in (tc.MS[index % 4], tc.MS[(index + 2) % 4]):
                p = tc.tile_rows(tc.coefficients(loop, m, n), R)
                p_stride = m + 3 if padded else m
                dp = DeviceArray.from_numpy(_blocks(p, 0, p_stride))
                for exp_rms in (0, 1):
                    mean, rms = (DeviceArray.from_numpy(np.full(R + 4, SENTINEL, T)) for _ in range(2))
                    run(L.dsp_poly_residual_rows, "poly_residual", *rows_args, exp_rms, dp.ptr, m, p_stride, mean.ptr, rms.ptr)
                    gm, gr = mean.to_numpy(), rms.to_numpy()
                    assert (gm[R:] == SENTINEL).all() and (gr[R:] == SENTINEL).all()
                    if exp_rms:
                        _exp_ok(gm[:R], gr[:R], w, p, T, (rows_type, n, m, padded))
                    else:
                        want = tc.emulate_residual(w, p, T, False)
                        assert tc.same(gm[:R], want[0]) and tc.same(gr[:R], want[1]), (rows_type, n, m, padded, _diff(gm[:R], want[0]), _diff(gr[:R], want[1]))
                    mean.free(), rms.free()
                dp.free()
            assert d.to_numpy().tobytes() == block.tobytes()  # (the rows are read, never written)
            d.free()
    assert {v[0] for v in vectors} == {True, False} and {v[1] for v in vectors} == {True, False}


# ---------------------------------------------------------------------------------------------------------------- 3. the fused launches
def _fused(loop, w, m, inv, **kw):
    """one launch of tc.program(...): {"out": logged rows, "pars_out": coefficients, "mean", "rms"} as far as the program stores them"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray, sync

    T = tc.LOOPS[loop]
    offset, row_stride = kw.get("offset", 0), kw.get("row_stride")
    R, n = w.shape[0], w.shape[1] - offset if row_stride is None else kw.pop("n")
    subtract = kw.pop("subtract", None)
    per_row = isinstance(subtract, np.ndarray)
    prog = tc.program(n, w.dtype, T, m=m, subtract="column" if per_row else subtract, **kw)
    chain = Chain(prog, compute_dtype=T)
    assert chain.kernel_name == tc.KERNEL and chain.geometry(R)["blocks"] == -(-R // 64)
    dev = {"w": DeviceArray.from_numpy(w)}
    if per_row:
        dev["bl"] = DeviceArray.from_numpy(subtract.astype(T))
    names = [i[0] for i in prog.io]
    if "inv" in names:
        dev["inv"] = DeviceArray.from_numpy(np.ascontiguousarray(inv).reshape(-1))
    for name, shape in (("out", (R, n)), ("pars_out", (R, m)), ("mean", (R,)), ("rms", (R,))):
        if name in names:
            dev[name] = DeviceArray.from_numpy(np.full(shape, SENTINEL, T))
    chain.execute(dev, R)
    sync()
    chain.check()
    got = {k: dev[k].to_numpy() for k in ("out", "pars_out", "mean", "rms") if k in dev}
    assert dev["w"].to_numpy().tobytes() == w.tobytes()
    chain.close()
    for d in dev.values():
        d.free()
    return got


@pytest.mark.parametrize("loop", list(tc.LOOPS))
def test_the_fused_launches_equal_the_calls_apart(loop):
    from dspeed_amd.processors import log_check, poly_diff, poly_exp_rms, poly_fit

    T = tc.LOOPS[loop]
    for index, (n, m) in enumerate(((3, 2), (63, 4), (64, 1), (65, 8), (129, 4), (129, 8), (64, 2))):
        R = tc.ROW_COUNTS[index % len(tc.ROW_COUNTS)]
        w = tc.tile_rows(tc.tail_rows(loop, n), R)
        fitter = poly_fit(n, m - 1)
        logged = log_check(w)
        _log_ok(logged, w, T, (n, m))
        pars = fitter(logged)
        assert tc.same(pars, tc.emulate_poly_fit(logged, fitter.inv, T)), (n, m)
        bad = np.isnan(logged).any(axis=1)
        assert np.isnan(pars[bad]).all() and (bad.any() or R == 1) and not bad.all()
        # log_check -> poly_fit: one pass, the logged row stored or not
        for store_log in (True, False):
            got = _fused(loop, w, m, fitter.inv, log=True, fit=True, store_log=store_log)
            assert tc.same(got["pars_out"], pars), (n, m, store_log, _diff(got["pars_out"], pars))
            assert ("out" in got) == store_log and (not store_log or tc.same(got["out"], logged))
        # ... -> the residuals of the logged row (poly_diff) and of the rows as loaded (poly_exp_rms): two passes, every choice of stores
        diff_apart, exp_apart = poly_diff(logged, pars), poly_exp_rms(w, pars)
        assert tc.same(diff_apart[0], tc.emulate_residual(logged, pars, T, False)[0]) and tc.same(diff_apart[1], tc.emulate_residual(logged, pars, T, False)[1]), (n, m)
        _exp_ok(*exp_apart, w, pars, T, (n, m))
        for store_log, store_pars in ((True, True), (False, False), (True, False), (False, True)):
            got = _fused(loop, w, m, fitter.inv, log=True, fit=True, resid="diff", resid_of="log", store_log=store_log, store_pars=store_pars)
            assert tc.same(got["mean"], diff_apart[0]) and tc.same(got["rms"], diff_apart[1]), (n, m, store_log, store_pars, _diff(got["mean"], diff_apart[0]))
            assert ("out" in got) == store_log and ("pars_out" in got) == store_pars
            assert (not store_log or tc.same(got["out"], logged)) and (not store_pars or tc.same(got["pars_out"], pars))
            got = _fused(loop, w, m, fitter.inv, log=True, fit=True, resid="exp", resid_of="rows", store_log=store_log, store_pars=store_pars)
            assert tc.same(got["mean"], exp_apart[0]) and tc.same(got["rms"], exp_apart[1]), (n, m, store_log, store_pars, _diff(got["mean"], exp_apart[0]))
        # a fit of the rows themselves with its residuals, no logarithm
        raw = fitter(w)
        got = _fused(loop, w, m, fitter.inv, fit=True, resid="diff", store_pars=True)
        want = tc.emulate_residual(w, raw, T, False)
        assert tc.same(got["pars_out"], raw) and tc.same(got["mean"], want[0]) and tc.same(got["rms"], want[1]), (n, m)


@pytest.mark.parametrize("rows_type", [np.float32, np.uint16, np.float64])
def test_a_subtraction_and_a_slice_folded_into_the_launch(rows_type):
    """LOAD of a slice with a non-zero start, BL_SUBTRACT, LOG_CHECK, POLY_FIT, POLY_EXP_RMS: one float subtraction as the rows are read -- the
    gufuncs apart, on bl_subtract's rows, give the same bits; a NaN baseline makes its row a NaN row, a baseline above the tail a bad one"""
    from dspeed_amd.processors import bl_subtract, log_check, poly_exp_rms, poly_fit

    loop = "f64" if rows_type is np.float64 else "f32"
    T = tc.LOOPS[loop]
    R, total, start, m = 70, 200, 71, 4
    n = total - start
    full = np.concatenate([np.full((R, start), 1234, np.float64), 1000 + tc.tile_rows(tc.tail_rows(loop, n)[:3].astype(np.float64), R)], axis=1)
    full = np.rint(full).astype(rows_type) if np.dtype(rows_type).kind in "iu" else full.astype(rows_type)
    bl = (990 + np.arange(R) % 7 * 0.25).astype(T)
    bl[5], bl[6] = np.nan, 5000
    fitter = poly_fit(n, m - 1)
    for baseline in (bl, 995.5):
        sub = bl_subtract(np.ascontiguousarray(full[:, start:]), baseline)
        logged = log_check(sub)
        pars = fitter(logged)
        apart = poly_exp_rms(sub, pars)
        for store_log in (True, False):
            got = _fused(loop, full, m, fitter.inv, n=n, offset=start, row_stride=total, log=True, fit=True, resid="exp", store_log=store_log, subtract=baseline)
            assert tc.same(got["pars_out"], pars) and tc.same(got["mean"], apart[0]) and tc.same(got["rms"], apart[1]), (rows_type, store_log, _diff(got["pars_out"], pars))
            assert not store_log or tc.same(got["out"], logged)
        if isinstance(baseline, np.ndarray):
            assert np.isnan(pars[[5, 6]]).all() and np.isnan(apart[1][[5, 6]]).all() and np.isfinite(pars[[0, 1, 2]]).all() and np.isfinite(apart[1][[0, 1, 2]]).all()


# ---------------------------------------------------------------------------------------------------------------- 4. the limits
def test_the_limits_at_the_gufuncs():
    from dspeed_amd.processors import poly_diff, poly_fit

    w = tc.tail_rows("f32", 65)
    with pytest.raises(NotImplementedError, match="poly_diff: at most 8 coefficients \\(9 given\\): a lane keeps one float64 accumulator each"):
        poly_diff(w, np.zeros(9, np.float32))
    with pytest.raises(NotImplementedError, match="poly_fit: at most 8 coefficients \\(9 given\\)"):
        poly_fit(65, 8)
    with pytest.raises(NotImplementedError, match="poly_fitter: \\(n - 1\\)\\*\\*\\(m - 1\\) must stay below 2\\*\\*63 \\(n = 600 samples, m = 8 coefficients\\)"):
        poly_fit(64, 7)(np.ones((2, 600), np.float32))
    with pytest.raises(ValueError, match="poly_fitter: poly_pars holds deg \\+ 1 = 4 coefficients \\(3 given\\)"):
        poly_fit(65, 3)(w, np.zeros((len(w), 3), np.float32))
    with pytest.raises(np.linalg.LinAlgError):
        poly_fit(2, 3)


# ---------------------------------------------------------------------------------------------------------------- 5. the recipe
M = "dspeed.processors"


def _tail_recipe(start):
    return {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "baseline", "wf_blsub"]},
            "wf_logged": {"function": "log_check", "module": M, "args": [f"wf_blsub[{start}:]", "wf_logged"]},
            "fit_pars": {"function": f"{M}.poly_fit", "args": ["wf_logged", "fit_pars(shape=4)"], "init_args": ["len(wf_logged)", 3]},
            "tail_mean, tail_rms": {"function": "poly_exp_rms", "module": f"{M}.poly_fit", "args": [f"wf_blsub[{start}:]", "fit_pars", "tail_mean", "tail_rms"]}}


def test_the_docstring_recipe():
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    n_rows, total, start = 70, 300, 171
    n = total - start
    tail = 1000 + tc.tile_rows(tc.tail_rows("f32", n)[:3].astype(np.float64), n_rows)
    w = np.rint(np.concatenate([np.full((n_rows, start), 1000.0), tail], axis=1)).astype(np.uint16)
    bl = (990 + np.arange(n_rows) % 5).astype(np.float32)
    bl[7] = 6000  # a baseline above the tail: not positive, NaNs all the way
    rows = (w.astype(np.float32) - bl[:, None])[:, start:]
    for outputs in (["fit_pars", "tail_mean", "tail_rms"], ["fit_pars", "tail_mean", "tail_rms", "wf_logged"]):
        chain, _, out = build_processing_chain({"outputs": outputs, "processors": _tail_recipe(start)}, {"waveform": WaveformInput(w, 16.0), "baseline": bl})
        chain.execute()
        assert [kernel for _what, kernel in chain.kernels()].count(tc.KERNEL) == 1
        pars = np.asarray(out["fit_pars"])
        assert pars.shape == (n_rows, 4) and pars.dtype == np.float32 and np.asarray(out["tail_mean"]).shape == (n_rows,)
        assert np.isnan(pars[7]).all() and np.isnan(out["tail_rms"][7]) and np.isfinite(np.delete(pars, 7, axis=0)).all()
        if "wf_logged" in outputs:
            logged = np.asarray(out["wf_logged"])
            _log_ok(logged, rows, np.float32, "recipe")
            assert tc.same(pars, tc.emulate_poly_fit(logged, tc.inverse(n, 3), np.float32)), _diff(pars, tc.emulate_poly_fit(logged, tc.inverse(n, 3), np.float32))
        _exp_ok(np.asarray(out["tail_mean"]), np.asarray(out["tail_rms"]), rows, pars, np.float32, "recipe")
        assert (np.asarray(out["tail_rms"])[0::3] < 20).all()  # the fit follows the slow tails: their residuals are the noise
