"""The register-resident energy kernel's guard reads and row loop: where a lane whose lagged window lies wholly below sample 0 reads its
zeros, and where in a row the next row's prefetch and the last row's pending result store sit.  Neither changes arithmetic, so every
case is held twice:

  * against the CPU oracle's processors at this chain's bar (tests/test_gpu_energy_even_pitch.py: NaN positions equal and
    |device - oracle| <= 1e-6 of the trapezoid's peak in the row);
  * against tests/golden/energy_row_pipeline.npz EXACTLY, bit patterns included: the outputs of the library as it was before the guard
    reads were moved, recorded on the device for these inputs by tools/record_energy_row_pipeline_fixture.py.  The fixture is recorded
    again only when the kernel's arithmetic changes on purpose.

Cases (tests/energy_row_pipeline_cases.py).  Guard: rows of 1024 and 2048 samples (their guard is longer than before), 4096 (the
benchmark's code), one case of 8192; lags that give each of the three streams in turn no lane that reads the guard, some, and all but one
of the lanes that hold samples; windows that end exactly at sample -1 and at sample 0; odd and even lags; trap_filter and
asym_trap_filter, float32 and int16 rows, modes 'l' and 'h' (the 4-point mode re-runs two 8-sample groups from the replay states the
kernel saves for it, and reads the lagged streams at run-time positions there).  Row loop, on 1024-sample rows (the build that
prefetches behind the staging) and on 4096-sample float32 rows (the build that prefetches and stores the pending result behind pass 2,
or at the end of a row that never gets there): launches of 1 row, of fewer rows than wavefronts, of exactly one, two and three rows per
wavefront, of two rows for some wavefronts and three for others -- every launch's geometry asserted; a NaN row as a wavefront's first,
middle and last row; a row whose pick-off time is out of range between two that are in range.  200 rows a guard case; a few thousand
rows a row-loop launch."""
import os

import numpy as np
import pytest

import energy_carry_cases as K
import energy_row_pipeline_cases as R
import oracle
from test_gpu_energy_even_pitch import KERNEL, TOL, _device, _ok, _recipe, _stride

pytestmark = pytest.mark.gpu
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "energy_row_pipeline.npz")
GUARD_CASES = R.guard_cases()
LOOP_IDS = [lid for lid, _len, _n, _mode in R.loop_launches(1)]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def run_guard_case(case, mode):
    """the device's output for one guard case and mode (also what the fixture's recorder calls)"""
    _cid, wf_len, dtype, trap, targs, _modes = case
    wf, bl, tp, _tau = K.rows(wf_len, dtype)
    return _device(wf, bl, tp, trap, targs, mode)


def loop_stride(wf_len):
    return _stride(wf_len, R.LOOP_TRAP, R.LOOP_GEOMETRY[wf_len])


def run_loop_launch(lid, strides):
    """(sample count, rows, mode, the device's output) of one row-loop launch; ``strides``: wavefronts of a full launch per sample count.
    The launch's geometry is asserted: `stride` wavefronts where the rows are as many or more, so that row r + stride follows row r on
    its wavefront and "exactly two rows each" is what runs; a wavefront per row, up to a workgroup's worth more, where they are fewer"""
    from dspeed_amd.processing_chain import build_processing_chain

    wf_len = {i: w for i, w, _n, _m in R.loop_launches(1)}[lid]
    stride = strides[wf_len]
    n, mode = {i: (n, m) for i, _w, n, m in R.loop_launches(stride)}[lid]
    wf, bl, tp = R.loop_rows(wf_len, n, stride)
    chain, _, out = build_processing_chain(_recipe(R.LOOP_TRAP, R.LOOP_GEOMETRY[wf_len], mode, K.TAU), {"waveform": wf, "baseline": bl, "t_pick": tp})
    chain._ensure()
    assert chain._chain.kernel_name == KERNEL, chain._chain.kernel_name
    g = chain.geometry(n)
    waves = g["blocks"] * g["waves_per_block"]
    assert waves == stride if n >= stride else n <= waves < n + g["waves_per_block"], (lid, g, n, stride)
    chain.execute()
    return wf_len, n, mode, np.array(out["trapEftp"])


def _hold_oracle(got, trapw, wf, tp, mode, wf_len, what):
    want = _ok(oracle.fixed_time_pickoff(trapw, tp, mode))
    nan = np.isnan(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), nan), (what, np.flatnonzero(np.isnan(got) != nan)[:8])
    expect_nan = ~((tp >= 0) & (tp <= wf_len - 1)) | np.isnan(wf.astype(F)).any(axis=1)
    assert np.array_equal(nan, expect_nan), (what, np.flatnonzero(nan != expect_nan)[:8])
    peak = np.max(np.abs(np.nan_to_num(trapw.astype(np.float64))), axis=1)[~nan]
    dev = np.abs(got[~nan].astype(np.float64) - want[~nan].astype(np.float64)) / np.where(peak > 0, peak, 1.0)
    print(f"{what}: worst |dev| / peak {dev.max() if dev.size else 0.0:.2e}")
    assert not ((peak == 0) & (got[~nan] != want[~nan])).any()  # no scale: exact
    assert dev.size == 0 or dev.max() <= TOL, (what, np.flatnonzero(dev > TOL)[:8], dev.max())


def _hold_recorded(got, rec, what):
    same = (got.view(np.uint32) == rec.view(np.uint32)) | (np.isnan(got) & np.isnan(rec))
    assert got.shape == rec.shape and np.array_equal(got, rec, equal_nan=True) and same.all(), (what, np.flatnonzero(~same)[:8])


@pytest.mark.parametrize("case", GUARD_CASES, ids=[c[0] for c in GUARD_CASES])
def test_guard_reads_against_the_oracle_and_exactly_against_the_recorded_outputs(case, golden):
    cid, wf_len, dtype, trap, targs, modes = case
    wf, bl, tp, _tau = K.rows(wf_len, dtype)
    trapw = _ok(getattr(oracle, trap)(_ok(oracle.pole_zero(_ok(oracle.bl_subtract(wf.astype(F), bl)), K.TAU)), *targs))
    for mode in modes:
        got = run_guard_case(case, mode)
        _hold_oracle(got, trapw, wf, tp, mode, wf_len, f"{cid} '{mode}'")
        _hold_recorded(got, golden[f"guard/{cid}/{mode}"], (cid, mode))


def test_the_geometries_reach_what_they_are_chosen_for():
    """(no device needed, but it belongs to the cases above)"""
    for wf_len in K.LENGTHS:
        C, lanes = K.chunk(wf_len), R.sample_lanes(wf_len)
        geo = R.guard_geometries(wf_len)
        per_stream = [{g[2][k] for g in geo} for k in range(3)]
        for k in range(3):  # no lane, some lanes, all lanes with samples but one
            assert 0 in per_stream[k] and lanes - 1 in per_stream[k] and any(0 < v < lanes - 1 for v in per_stream[k]), (wf_len, k, per_stream[k])
        lags = [lag for trap, targs, _l in geo for lag in K.lags_of(trap, targs)]
        assert any(lag >= C and lag % C == 0 for lag in lags) and any(lag % C == C - 1 for lag in lags)  # a window ends at sample -1, at sample 0
        for k in range(3):
            assert {K.lags_of(trap, targs)[k] & 1 for trap, targs, _l in geo} == {0, 1}
        for trap, targs, _l in geo:
            assert K.lags_of(trap, targs)[2] <= wf_len
    assert {(c[1], np.dtype(c[2]).name) for c in GUARD_CASES} >= {(n, t) for n in (1024, 2048, 4096) for t in ("float32", "int16")}
    assert any(c[1] == 8192 for c in GUARD_CASES) and all("l" in c[5] for c in GUARD_CASES) and sum("h" in c[5] for c in GUARD_CASES) >= 12


@pytest.mark.parametrize("lid", LOOP_IDS)
def test_row_loop_against_the_oracle_and_exactly_against_the_recorded_outputs(lid, golden):
    strides = {w: loop_stride(w) for w in R.LOOP_GEOMETRY}
    wf_len, n, mode, got = run_loop_launch(lid, strides)
    stride = strides[wf_len]
    wf, bl, tp = R.loop_rows(wf_len, n, stride)
    rec = golden[f"loop/{lid}"]
    assert len(rec) == n, f"the fixture was recorded on a device whose launch has {int(golden[f'loop/stride-{wf_len}'])} wavefronts, this one has {stride}"
    # the special rows are where the docstring says: NaN as a wavefront's middle, first and last row, a time out of range between two in range
    finite = lambda *rows: not np.isnan(got[list(rows)]).any()  # noqa: E731
    if n >= 2 * stride:
        assert np.isnan(got[R.W_NAN_MID + stride]) and finite(R.W_NAN_MID)
        assert np.isnan(got[R.W_NAN_FIRST]) and finite(R.W_NAN_FIRST + stride)
        assert np.isnan(got[R.W_RANGE + stride]) and finite(R.W_RANGE)
    if n > 2 * stride:
        assert R.W_NAN_LAST + 2 * stride < n
        assert finite(R.W_NAN_MID + 2 * stride, R.W_NAN_FIRST + 2 * stride, R.W_RANGE + 2 * stride)
        assert np.isnan(got[R.W_NAN_LAST + 2 * stride]) and finite(R.W_NAN_LAST, R.W_NAN_LAST + stride)
    trapw = _ok(oracle.trap_filter(_ok(oracle.pole_zero(_ok(oracle.bl_subtract(wf, bl)), K.TAU)), *R.LOOP_GEOMETRY[wf_len]))
    _hold_oracle(got, trapw, wf, tp, mode, wf_len, f"{lid} ({n} rows of {wf_len} on {stride} wavefronts) '{mode}'")
    _hold_recorded(got, rec, lid)
