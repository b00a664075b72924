"""The register-resident energy kernel at its even lane pitch (C = len/64 + 2 samples per lane, chunks of (C - 2) / 8 groups of 8 samples
and a two-sample tail, lagged streams read as aligned 8-byte pairs with one copy of the replay per lag-parity case): every row against the
CPU oracle's processors, none left out.

Bar, the project's own for this chain: NaN positions equal and |device - oracle| <= 1e-6 of the trapezoid's peak in that row (as
tests/test_gpu_chain.test_energy_pickoff_position_sweep and tests/test_gpu_row_families hold it: the pick-off times here sweep the whole row,
and the filter's rounding noise does not shrink where its output is near zero).

What the cases are chosen for:
  * 1024-sample rows (C = 18, the smallest length the kernel takes), 130 of them, and one small case at 2048 / 4096 / 8192: these are the
    per-row cases, a wavefront filters at most one row in them (the launch has a wavefront per row up to 8 per CU);
  * launches of two rows per wavefront and 104 more (a few thousand 1024-sample rows; the count comes from the chain's launch geometry and
    the test asserts that it loops): wavefront w filters rows w, w + stride, w + 2 stride in one LDS region that it zeroes once.  What a row
    leaves there -- pass 2's tail in the virtual samples above len, the side arrays, the capture buffer -- must not reach the next: the
    pick-off positions of the list below go to the rows of every round, rotated so that a wavefront meets another one each round; a NaN
    row and a constant row sit in the first round and in the second, directly before clean rows on their wavefronts; four lag-parity
    classes, modes 'l', 'n', 'h', float32 and int16 rows.  A test of its own puts an infinite-sample row (whose pass 2 leaves NaN in the
    virtual samples) into the first round or the second, directly before a clean row that picks off in the lane that held the NaN;
  * (rise, flat) from all four parity classes of the lags rise, rise + flat, 2 rise + flat, and lags that are exact multiples of C and one
    either side (the speculative carries are then captured on, just before and just after a chunk boundary and inside the two-sample tail);
    asym_trap_filter's fall time makes the third lag's parity free: all eight classes;
  * pick-off times at 0, 0.5, C-3 .. C+0.5 (last group, the tail's two samples, the next lane's first), in the last lane that holds samples,
    len-1.5, len-1 and out of range; modes 'l', 'n', 'h' (the 4-point mode re-runs the tail group and a lane's first group);
  * the three trapezoids, float32 / int16 / uint16 rows, a time constant per event;
  * a row with a NaN sample, a constant row, and a row with an infinite sample (the reference raises there: so must the chain, naming the row)."""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
F = np.float32
M = "dspeed.processors"
TAU = 1716.28
TOL = 1e-6
KERNEL = "dsp_energy_rr_kernel"


def _ok(r):
    out, rc = r
    assert rc == 0, rc
    return out


def _pick_times(n, wf_len, rng):
    """the positions the docstring lists, each also with a fraction, then random ones"""
    C = wf_len // 64 + 2
    last = ((wf_len - 1) // C) * C  # first sample of the last lane that holds any
    fixed = [0.0, 0.5, 1.0, C - 3, C - 2.5, C - 2, C - 1.75, C - 1, C - 0.5, C, C + 0.5, 2 * C - 2, 2 * C - 1, 2 * C - 0.25, 7 * C + 8, 7 * C + 15.5,
             last - 1, last - 0.5, last, last + 1.5, wf_len - 2, wf_len - 1.5, wf_len - 1, wf_len - 0.5, wf_len + 3.0, -1.0, np.nan]
    tp = np.empty(n, F)
    tp[:len(fixed)] = fixed[:n]
    rest = n - len(fixed)
    if rest > 0:
        r = rng.uniform(0, wf_len - 1, rest)
        r[::3] = np.floor(r[::3])  # integer times take their own return in the pick-off
        tp[len(fixed):] = r
    return tp, len(fixed)


@functools.lru_cache(maxsize=None)
def _rows(n, wf_len, dtype, stride=0):
    """pulses on a pedestal with noise; three special rows among them.  Shared and left unchanged.  ``stride``: rows a launch filters per
    round (row r + stride follows row r on its wavefront), 0 where every row has a wavefront of its own"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1000 * wf_len + n + ord(dtype.char))
    i = np.arange(wf_len, dtype=np.float64)[None, :]
    ped = rng.uniform(-3000, 3000, (n, 1)) + (20000 if dtype == np.uint16 else 0) + (9000 if dtype == F else 0)
    amp = rng.uniform(500, 15000, (n, 1))
    t0 = np.floor(rng.uniform(0.05, 0.9, (n, 1)) * wf_len)
    x = ped + amp * np.exp(-(i - t0) / TAU) * (i >= t0) + 5.0 * rng.standard_normal((n, wf_len))
    x[5] = ped[5]  # a constant row
    if stride:
        x[stride + 11] = ped[stride + 11]
    wf = (np.rint(x) if dtype.kind in "iu" else x).astype(dtype)
    if dtype == F:
        wf[9, (wf_len // 64 + 2) * 3 + wf_len // 64] = np.nan  # a NaN sample, in a lane's two-sample tail
        if stride:
            wf[stride + 3, wf_len - 1] = np.nan  # and one in a second-round row, in the lane that also holds virtual samples
    bl = ped[:, 0].astype(F)
    tp, nfixed = _pick_times(n, wf_len, rng)
    for k in range(1, n // stride + 1 if stride else 0):  # the listed positions again in every later round, on other wavefronts' turns
        tp[k * stride:k * stride + nfixed] = np.roll(tp[:nfixed], 7 * k)
    for a in (wf, bl, tp):
        a.setflags(write=False)
    return wf, bl, tp


def _recipe(trap, targs, mode, tau):
    return {"outputs": ["trapEftp"], "processors": {
        "wf_blsub": f"{M}.bl_subtract(waveform, baseline, wf_blsub)",
        "wf_pz": f"{M}.pole_zero(wf_blsub, {tau}, wf_pz)",
        "wf_trap": {"function": trap, "module": M, "args": ["wf_pz", *[str(a) for a in targs], "wf_trap"]},
        "trapEftp": {"function": "fixed_time_pickoff", "module": M, "args": ["wf_trap", "t_pick", f"'{mode}'", "trapEftp"]}}}


def _stride(wf_len, trap="trap_filter", targs=(100, 31)):
    """rows the kernel's launch filters per round on this device: its wavefronts when there are more rows than those"""
    from dspeed_amd.processing_chain import build_processing_chain

    z = np.zeros((4, wf_len), F)
    chain, _, _out = build_processing_chain(_recipe(trap, targs, "l", TAU), {"waveform": z, "baseline": z[:, 0].copy(), "t_pick": z[:, 0].copy()})
    chain._ensure()
    assert chain._chain.kernel_name == KERNEL, chain._chain.kernel_name
    g = chain.geometry(1 << 30)
    return g["blocks"] * g["waves_per_block"]


def _device(wf, bl, tp, trap, targs, mode, tau=None, stride=0):
    from dspeed_amd.processing_chain import build_processing_chain

    tb = {"waveform": wf, "baseline": bl, "t_pick": tp}
    if tau is not None:
        tb["tau"] = tau
    chain, _, out = build_processing_chain(_recipe(trap, targs, mode, TAU if tau is None else "tau"), tb)
    chain._ensure()
    assert chain._chain.kernel_name == KERNEL, chain._chain.kernel_name
    if stride:  # this launch has `stride` wavefronts and every one of them filters two rows or three
        g = chain.geometry(len(wf))
        assert g["blocks"] * g["waves_per_block"] == stride and len(wf) > 2 * stride, (g, len(wf), stride)
    chain.execute()
    return np.array(out["trapEftp"])


@functools.lru_cache(maxsize=None)
def _filtered(n, wf_len, dtype, trap, targs, per_event=False, stride=0):
    """the oracle's trapezoid rows (float32 loop, as the reference picks it for 16-bit rows) and the time constants used"""
    wf, bl, _tp = _rows(n, wf_len, dtype, stride)
    xs = _ok(oracle.bl_subtract(wf.astype(F), bl))
    if per_event:
        tau = np.random.default_rng(n + wf_len).uniform(800, 2500, n).astype(F)
        pz = np.concatenate([_ok(oracle.pole_zero(xs[r:r + 1], float(tau[r]))) for r in range(n)])
    else:
        tau = None
        pz = _ok(oracle.pole_zero(xs, TAU))
    return _ok(getattr(oracle, trap)(pz, *targs)), tau


def _hold(n, wf_len, dtype, trap, targs, modes="lnh", per_event=False, stride=0):
    wf, bl, tp = _rows(n, wf_len, dtype, stride)
    trapw, tau = _filtered(n, wf_len, dtype, trap, tuple(targs), per_event, stride)
    peak = np.max(np.abs(np.nan_to_num(trapw.astype(np.float64))), axis=1)
    for mode in modes:
        want = _ok(oracle.fixed_time_pickoff(trapw, tp, mode))
        got = _device(wf, bl, tp, trap, targs, mode, tau, stride)
        assert got.shape == want.shape
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (mode, np.flatnonzero(np.isnan(got) != nan)[:8])
        expect_nan = ~((tp >= 0) & (tp <= wf_len - 1)) | np.isnan(wf.astype(F)).any(axis=1)  # out-of-range and NaN times, the NaN row: nothing else
        assert np.array_equal(nan, expect_nan), (mode, np.flatnonzero(nan != expect_nan)[:8])
        dev = np.abs(got[~nan].astype(np.float64) - want[~nan].astype(np.float64)) / np.where(peak[~nan] > 0, peak[~nan], 1.0)
        flat_rows = peak[~nan] == 0
        print(f"len={wf_len} {np.dtype(dtype).name} {trap}{tuple(targs)} '{mode}': worst |dev| / peak {dev.max():.2e}")
        assert not (flat_rows & (got[~nan] != want[~nan])).any()  # no scale: exact
        assert dev.max() <= TOL, (mode, np.flatnonzero(dev > TOL)[:8], dev.max())


# lag parity (rise & 1, flat & 1) in all four classes, then lags that are multiples of C = 18 and one either side
LAGS_1024 = [(100, 30), (101, 30), (100, 31), (101, 31)] + [(r, f) for r in (17, 18, 19, 36) for f in (18, 19)]


@pytest.mark.parametrize("rise,flat", LAGS_1024)
def test_lag_parity_and_chunk_boundaries_1024(rise, flat):
    _hold(130, 1024, F, "trap_filter", (rise, flat))


# ---- more rows than wavefronts: every wavefront filters two rows, the first 104 a third
LOOP_EXTRA = 104


@pytest.mark.parametrize("dtype,trap,targs", [(F, "trap_filter", (100, 30)), (F, "trap_filter", (101, 30)), (F, "trap_norm", (18, 19)),
                                              (np.int16, "asym_trap_filter", (101, 31, 40))], ids=str)
def test_wavefronts_that_filter_several_rows_1024(dtype, trap, targs):
    """lags even-even-even, odd-odd-even, even-odd-odd (a lag of exactly C), odd-even-even; all three pick-off modes"""
    stride = _stride(1024, trap, targs)
    _hold(2 * stride + LOOP_EXTRA, 1024, dtype, trap, targs, stride=stride)


@pytest.mark.parametrize("rnd", [0, 1], ids=["first_row", "second_row"])
@pytest.mark.parametrize("mode,rise,flat", [("h", 101, 30), ("l", 100, 31)])
def test_row_after_an_infinite_sample_row_on_the_same_wavefront(mode, rise, flat, rnd):
    """The infinite sample sits in the last lane that holds samples: pass 2 writes inf, then NaN, into that lane's two virtual samples and
    into everything above.  The row named is that one; the rows that follow it on its wavefront (and all others) are what the oracle says."""
    from dspeed_amd.chain import Chain, energy_chain_program
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.errors import DSPFatal

    stride = _stride(1024)
    n = 2 * stride + LOOP_EXTRA
    wf, bl, tp = (a.copy() for a in _rows(n, 1024, F, stride))
    wf = np.nan_to_num(wf, nan=0.0)
    tp[~((tp >= 0) & (tp <= 1023))] = 500.25  # (times out of range are the other tests' matter: here every row but one has a value)
    bad = rnd * stride + 41  # rows bad + stride (and bad + 2 stride, when bad is a first row) follow it on its wavefront
    assert bad + stride < n
    wf[bad, 1010] = np.inf
    tp[bad + stride] = 1021.5  # the row right after it picks off in the lane whose tail held the NaN
    ch = Chain(energy_chain_program(1024, TAU, rise, flat, mode), "energy")
    assert ch.kernel_name == KERNEL
    g = ch.geometry(n)
    assert g["blocks"] * g["waves_per_block"] == stride
    bufs = {"waveform": DeviceArray.from_numpy(wf), "baseline": DeviceArray.from_numpy(bl), "t_pick": DeviceArray.from_numpy(tp),
            "trapEftp": DeviceArray((n,), F)}
    with pytest.raises(DSPFatal) as ei:
        ch.execute(bufs, n)
        ch.check()
    assert ei.value.wf_range == range(bad, bad + 1)
    got = bufs["trapEftp"].to_numpy()
    keep = np.arange(n) != bad
    want = _ok(oracle.chain_energy(wf[keep], bl[keep], tp[keep], TAU, rise, flat, mode))
    peak = np.max(np.abs(_ok(oracle.chain_pz_trap(wf[keep] - bl[keep, None], TAU, rise, flat))), axis=1)
    nan = np.isnan(want)
    assert np.isnan(got[bad]) and np.array_equal(np.isnan(got[keep]), nan), np.flatnonzero(np.isnan(got[keep]) != nan)[:8]
    assert not nan[bad + stride - 1]  # (index among the kept rows of row bad + stride)
    assert np.all(np.abs(got[keep][~nan].astype(np.float64) - want[~nan]) <= TOL * peak[~nan])  # (constant rows have no scale: exact)


@pytest.mark.parametrize("wf_len,rise,flat", [(2048, 67, 34), (4096, 625, 188), (4096, 66, 67), (8192, 1251, 130)])
def test_longer_rows(wf_len, rise, flat):
    _hold(70, wf_len, F, "trap_filter", (rise, flat))


@pytest.mark.parametrize("dtype", [F, np.int16, np.uint16], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("trap,targs", [("trap_norm", (100, 31)), ("trap_norm", (18, 19)), ("asym_trap_filter", (101, 30, 40)),
                                        ("asym_trap_filter", (36, 18, 19)), ("trap_filter", (19, 18))], ids=str)
def test_trapezoids_and_row_types(trap, targs, dtype):
    _hold(130, 1024, dtype, trap, targs)


@pytest.mark.parametrize("fall", [40, 41])
@pytest.mark.parametrize("rise,flat", [(100, 30), (101, 30), (100, 31), (101, 31)])
def test_asym_trap_all_eight_parity_classes(rise, flat, fall):
    _hold(130, 1024, F, "asym_trap_filter", (rise, flat, fall), modes="lh")


@pytest.mark.parametrize("dtype,trap,targs", [(F, "trap_filter", (101, 30)), (np.int16, "trap_norm", (18, 19))], ids=str)
def test_time_constant_per_event(dtype, trap, targs):
    _hold(130, 1024, dtype, trap, targs, per_event=True)


@pytest.mark.parametrize("wf_len", [1024, 4096])
def test_infinite_sample_raises_like_the_reference_and_names_the_row(wf_len):
    """inf - c inf is NaN two samples on: pole_zero.py:76-77 raises, the oracle returns PZ_NAN, the kernel reports the row"""
    from dspeed_amd.chain import Chain, energy_chain_program
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.errors import DSPFatal

    wf, bl, tp = (a.copy() for a in _rows(70, wf_len, F))
    wf = np.nan_to_num(wf, nan=0.0)
    tp[:] = wf_len // 2 + 0.5
    C = wf_len // 64 + 2
    wf[41, 20 * C + C - 2] = np.inf
    _out, rc = oracle.pole_zero(_ok(oracle.bl_subtract(wf[41:42], bl[41:42])), TAU)
    assert rc == 1
    ch = Chain(energy_chain_program(wf_len, TAU, 100, 31, "l"), "energy")
    assert ch.kernel_name == KERNEL
    bufs = {"waveform": DeviceArray.from_numpy(wf), "baseline": DeviceArray.from_numpy(bl), "t_pick": DeviceArray.from_numpy(tp),
            "trapEftp": DeviceArray((len(wf),), F)}
    with pytest.raises(DSPFatal) as ei:
        ch.execute(bufs, len(wf))
        ch.check()
    assert ei.value.wf_range == range(41, 42)
    got = bufs["trapEftp"].to_numpy()  # the other rows are what they are without it
    keep = np.arange(len(wf)) != 41
    want = _ok(oracle.chain_energy(wf[keep], bl[keep], tp[keep], TAU, 100, 31, "l"))
    peak = np.max(np.abs(_ok(oracle.chain_pz_trap(wf[keep] - bl[keep, None], TAU, 100, 31))), axis=1)
    assert np.isnan(got[41]) and not np.isnan(got[keep]).any()
    assert np.all(np.abs(got[keep].astype(np.float64) - want) <= TOL * peak)  # (the constant row has no scale: exact)
