"""The register-resident energy kernel's row-invariant work done once: the carry plan the host delivers in the form the kernel uses (pair
address, side-array element or a word of 0.0f, count pn; "all eight running prefixes, then pick one") and the tail as a build per
pick-off mode class (two-point modes n f c l i in straight-line selects, the 4-point mode h with its re-runs).  None of it changes arithmetic, so every case is held twice:

  * against the CPU oracle's processors at this chain's bar (tests/test_gpu_energy_even_pitch.py: NaN positions equal and
    |device - oracle| <= 1e-6 of the trapezoid's peak in the row);
  * against tests/golden/energy_carry_plan.npz EXACTLY (numpy.array_equal with equal_nan): the outputs of the library as it was before this
    change, recorded on the device for these inputs by tools/record_energy_carry_fixture.py.  The fixture is regenerated only when the
    kernel's arithmetic changes on purpose.

Cases (tests/energy_carry_cases.py): capture points 0, 1, 8, 9, C - 2, C - 1 of some lag at every length the kernel takes, all parities of
the lags, a lag below C, lags that leave most lanes' windows below sample 0, the three trapezoids, float32 / int16 / uint16 rows, a time
constant per event, two replay sub-chains; every pick-off mode with times at 0, len - 1, len - 1.5, just outside both ends, NaN, whole and
fractional, and i0 at chunk offsets C - 3, C - 2, C - 1 and 0; rows with a NaN sample, with zeros and negative zeros only, constant.  A few
hundred rows each, a wavefront per row; one launch in which every wavefront filters two or three rows (the plan is held in registers
across the row loop)."""
import os

import numpy as np
import pytest

import energy_carry_cases as K
import oracle
from test_gpu_energy_even_pitch import KERNEL, TOL, _device, _ok, _stride

pytestmark = pytest.mark.gpu
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "energy_carry_plan.npz")
CASES = K.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_trapezoids = {}


def _trapezoid(wf_len, dtype, trap, targs, per_event):
    key = (wf_len, np.dtype(dtype).name, trap, targs, per_event)
    if key not in _trapezoids:
        wf, bl, _tp, tau = K.rows(wf_len, dtype)
        xs = _ok(oracle.bl_subtract(wf.astype(F), bl))
        if per_event:
            pz = np.concatenate([_ok(oracle.pole_zero(xs[r:r + 1], float(tau[r]))) for r in range(len(xs))])
        else:
            pz = _ok(oracle.pole_zero(xs, K.TAU))
        _trapezoids[key] = _ok(getattr(oracle, trap)(pz, *targs))
    return _trapezoids[key]


def run_case(case, mode):
    """the device's output for one case and mode (also what the fixture's recorder calls)"""
    _cid, wf_len, dtype, trap, targs, _modes, per_event, S = case
    wf, bl, tp, tau = K.rows(wf_len, dtype)
    old = os.environ.get("DSPEED_HIP_VARIANT")
    if S == 2:
        os.environ["DSPEED_HIP_VARIANT"] = "8"  # read when the chain is planned
    try:
        return _device(wf, bl, K.times_for(mode, tp), trap, targs, mode, tau if per_event else None)
    finally:
        if S == 2:
            if old is None:
                del os.environ["DSPEED_HIP_VARIANT"]
            else:
                os.environ["DSPEED_HIP_VARIANT"] = old


def _hold_oracle(got, trapw, wf, tp, mode, wf_len, what):
    want = _ok(oracle.fixed_time_pickoff(trapw, tp, mode))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.flatnonzero(np.isnan(got) != nan)[:8])
    expect_nan = ~((tp >= 0) & (tp <= wf_len - 1)) | np.isnan(wf.astype(F)).any(axis=1)
    assert np.array_equal(nan, expect_nan), (what, np.flatnonzero(nan != expect_nan)[:8])
    peak = np.max(np.abs(np.nan_to_num(trapw.astype(np.float64))), axis=1)[~nan]
    dev = np.abs(got[~nan].astype(np.float64) - want[~nan].astype(np.float64)) / np.where(peak > 0, peak, 1.0)
    print(f"{what}: worst |dev| / peak {dev.max():.2e}")
    assert not ((peak == 0) & (got[~nan] != want[~nan])).any()  # no scale: exact
    assert dev.max() <= TOL, (what, np.flatnonzero(dev > TOL)[:8], dev.max())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_the_oracle_and_exactly_against_the_recorded_outputs(case, golden):
    cid, wf_len, dtype, trap, targs, modes, per_event, _S = case
    wf, _bl, tp, _tau = K.rows(wf_len, dtype)
    trapw = _trapezoid(wf_len, dtype, trap, targs, per_event)
    for mode in modes:
        got = run_case(case, mode)
        _hold_oracle(got, trapw, wf, K.times_for(mode, tp), mode, wf_len, f"{cid} '{mode}'")
        rec = golden[f"{cid}/{mode}"]
        same = (got.view(np.uint32) == rec.view(np.uint32)) | (np.isnan(got) & np.isnan(rec))
        assert np.array_equal(got, rec, equal_nan=True) and same.all(), (cid, mode, np.flatnonzero(~same)[:8])  # (the sign of a zero included)


def test_the_cases_reach_every_capture_point_they_are_chosen_for():
    for wf_len in K.LENGTHS:
        C = K.chunk(wf_len)
        seen = {K.capture_point(C, 1, 0, lag)[0] for g in K.carry_geometries(wf_len)[:-1] for lag in K.lags_of("trap_filter", g)}
        assert set(K.edge_points(C)) <= seen, (wf_len, seen)
        assert {(r & 1, f & 1) for r, f in K.carry_geometries(wf_len)} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("mode,rise,flat", [("l", 17, 11), ("h", 18, 19), ("n", 20, 7)])
def test_wavefronts_that_filter_several_rows(mode, rise, flat):
    """more rows than wavefronts: what the kernel keeps across its row loop (the plan's addresses, the packed counts) serves every row"""
    stride = _stride(1024)
    n = 2 * stride + 104
    wf, bl, tp, _tau = K.rows(1024, F, n)
    got = _device(wf, bl, tp, "trap_filter", (rise, flat), mode, None, stride)
    trapw = _ok(oracle.trap_filter(_ok(oracle.pole_zero(_ok(oracle.bl_subtract(wf, bl)), K.TAU)), rise, flat))
    _hold_oracle(got, trapw, wf, tp, mode, 1024, f"looping launch '{mode}' ({rise}, {flat})")


def _raises_for_row(program, wf, bl, tp, row):
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.errors import DSPFatal

    ch = Chain(program, "energy")
    assert ch.kernel_name == KERNEL
    bufs = {"waveform": DeviceArray.from_numpy(wf), "baseline": DeviceArray.from_numpy(bl), "t_pick": DeviceArray.from_numpy(tp),
            "trapEftp": DeviceArray((len(wf),), F)}
    with pytest.raises(DSPFatal) as ei:
        ch.execute(bufs, len(wf))
        ch.check()
    assert ei.value.wf_range == range(row, row + 1)
    return str(ei.value), bufs["trapEftp"].to_numpy()


MODE_I_ERRORS = [(1024, 57, 300.5), (4096, 3, 4094.25), (8192, 190, 0.5)]


def mode_i_error_launch(wf_len, row, t):
    """whole-number times in every row but one (the kernel names the first row it meets: with one such row the name is that row)"""
    from dspeed_amd.chain import energy_chain_program

    wf, bl, tp, _tau = K.rows(wf_len, F)
    wf = np.nan_to_num(wf, nan=0.0)
    tp = np.floor(np.nan_to_num(tp, nan=7.0)).astype(F)
    tp[row] = t
    return _raises_for_row(energy_chain_program(wf_len, K.TAU, 100, 31, "i"), wf, bl, tp, row)


@pytest.mark.parametrize("wf_len,row,t", MODE_I_ERRORS)
def test_mode_i_with_a_time_between_samples_raises_and_names_the_row(wf_len, row, t, golden):
    """fixed_time_pickoff.py raises for mode 'i' and a non-integer time; the kernel reports that row, the others keep their values"""
    text, got = mode_i_error_launch(wf_len, row, t)
    assert "integer t_in" in text
    assert np.isnan(got[row])
    assert np.array_equal(got, golden[f"mode-i-error-{wf_len}"], equal_nan=True)


def test_infinite_sample_row_is_named():
    """(the pole-zero output turns NaN two samples after an infinite one: pole_zero.py:76-77 raises, the kernel names the row)"""
    from dspeed_amd.chain import energy_chain_program

    wf, bl, tp, _tau = K.rows(1024, F)
    wf = np.nan_to_num(wf, nan=0.0)
    wf[41, 20 * K.chunk(1024) + 7] = np.inf
    _raises_for_row(energy_chain_program(1024, K.TAU, 17, 11, "l"), wf, bl, np.nan_to_num(tp, nan=7.0), 41)
