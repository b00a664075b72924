"""The register-resident energy kernel's picks at run-time positions: the replay's output at the two pick-off samples, the eight samples of
a carry's capture group and the prefix sum in front of it.  How the kernel fetches them (an indexed register move or a trip through LDS) is
no arithmetic, so every case is held twice:

  * against the CPU oracle's processors at this chain's bar (tests/test_gpu_energy_even_pitch.py: NaN positions equal and
    |device - oracle| <= 1e-6 of the trapezoid's peak in the row);
  * against tests/golden/energy_register_picks.npz EXACTLY, bit pattern for bit pattern: the outputs of the library as it was while all three
    picks still went through LDS, recorded on the device for these inputs by tools/record_energy_register_picks_fixture.py.  The fixture is
    regenerated only when the kernel's arithmetic changes on purpose.

Cases (tests/energy_register_picks_cases.py), rows of 1024 samples (C = 18, the smallest build) and of 4096 float32 samples (C = 66, the
build with the late prefetch), 101 / 231 rows a launch, a wavefront per row (fewer rows than the device has wavefronts):

  * pick-off positions: i0 on every offset of every 16-sample capture block of lane 0, lane 1, a middle lane and the last lane that holds
    samples (lane 63's chunk is virtual samples at this pitch), so the first and the last block of a chunk, both samples of the two-sample
    tail, i0 and i0 + 1 in different blocks and in different lanes; whole-number times; len - 1, which has no second sample; a row with a
    NaN sample between good rows;
  * carry plans: (rise, flat) that put a lag's capture point on every sample 0 .. C - 1 of the chunk at 1024 -- group 0 with nothing in front
    of it and every count pn 0 .. 8, the tail group whose capture reaches past the chunk -- and on both ends of every group at 4096; all four
    lag-parity cases of trap_filter, an asym_trap_filter whose third lag's parity is not the sum of the other two's, trap_norm;
  * builds: modes n f c l (two-point) and h (4-point), int16 rows, a time constant per event."""
import os

import numpy as np
import pytest

import energy_register_picks_cases as K
import oracle
from test_gpu_energy_carry_plan import _hold_oracle
from test_gpu_energy_even_pitch import _device, _ok

pytestmark = pytest.mark.gpu
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "energy_register_picks.npz")
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
    _cid, wf_len, dtype, trap, targs, _modes, per_event = case
    wf, bl, tp, tau = K.rows(wf_len, dtype)
    return _device(wf, bl, tp, trap, targs, mode, tau if per_event else None)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_the_oracle_and_bit_for_bit_against_the_recorded_outputs(case, golden):
    cid, wf_len, dtype, trap, targs, modes, per_event = case
    wf, _bl, tp, _tau = K.rows(wf_len, dtype)
    trapw = _trapezoid(wf_len, dtype, trap, targs, per_event)
    for mode in modes:
        got = run_case(case, mode)
        _hold_oracle(got, trapw, wf, tp, mode, wf_len, f"{cid} '{mode}'")
        rec = golden[f"{cid}/{mode}"]
        assert got.dtype == rec.dtype == F and got.shape == rec.shape
        same = got.view(np.uint32) == rec.view(np.uint32)  # (the sign of a zero and a NaN's payload included)
        assert same.all(), (cid, mode, np.flatnonzero(~same)[:8], got[~same][:8], rec[~same][:8])


def test_the_cases_reach_every_position_they_are_chosen_for():
    for wf_len in K.LENGTHS:
        C = K.chunk(wf_len)
        tp = K.pick_times(wf_len)
        i0 = np.floor(tp).astype(int)
        frac = tp != np.floor(tp)
        for lane in (0, K.last_lane(wf_len)):
            offs = set((i0[(i0 // C == lane) & frac] % C).tolist())
            assert offs == {o for o in range(C) if lane * C + o + 1 <= wf_len - 1}, (wf_len, lane, offs)
        offs = set((i0[frac] % C).tolist())
        assert {15, C - 2, C - 1} <= offs and (wf_len == 1024 or {31, 47, 63} <= offs)  # i0 / i0 + 1 astride blocks, the tail, lanes
        assert (tp == wf_len - 1).any() and (~frac).sum() >= 10
        seen, pns, par = set(), set(), set()
        for g in K.carry_geometries(wf_len):
            par.add((g[0] & 1, g[1] & 1))
            for lag in K.lags_of("trap_filter", g):
                r = K.capture_point(C, 1, 0, lag)[0]
                seen.add(r)
                pns.add(r - 8 * ((max(r, 1) - 1) // 8))
        assert set(K.wanted_capture_points(wf_len)) <= seen, (wf_len, seen)
        assert pns >= set(range(9)) and par == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert C - 1 in seen and 0 in seen  # the tail group (its capture reaches 6 past the chunk); nothing at all in front
    wf, _bl, _tp, _tau = K.rows(1024, F)
    nan = np.isnan(wf).any(axis=1)
    assert nan[K.NAN_ROW] and nan.sum() == 1 and 0 < K.NAN_ROW < len(wf) - 1
    trap, targs = next((c[3], c[4]) for c in CASES if c[3] == "asym_trap_filter")
    lags = K.lags_of(trap, targs)
    assert (lags[2] & 1) != ((lags[0] + lags[1]) & 1)
