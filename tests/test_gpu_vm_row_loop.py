"""The waveform interpreter's row loop: rows that follow another row on their wavefront.

dsp_vm_kernel's wavefronts are persistent: one clears its LDS region once and then runs row after row on it, so from its second row on
a row finds the guards, pads, shared regions, registers and scratch area as its predecessor left them.  Every case of
tests/vm_row_loop_cases.py is one program kept whole on the interpreter and one launch of 3 S + S // 2 rows, S the rows the launch
takes per round: round 0 probes, round 1 poison rows (NaN, infinities, +-3e38, zeros, denormals, NaN per-event values, times outside
the row, thresholds nothing reaches), round 2 the probes of round 0 again, round 3 (half of the wavefronts) other probes.  Held:

  1. the geometry: blocks x wavefronts per block / team == S, so that row r + S did follow row r on its wavefront;
  2. no memory of the previous row: every output of a round-2 row equals its round-0 twin bit for bit (no reference, no tolerance);
  3. every row against the oracle, at the bars of test_gpu_processors.py: bit-exact for indices, thresholds, min/max, pick-offs,
     bl_subtract, the DWT and one-operation expressions; FILTER_TOL of the row's peak for float32 filter outputs and what is read off
     them; FILTER_TOL_F64 / DPZ_TOL_F64 in the float64 loop; NaN and infinity positions equal;
  4. the team program once more on the same handle: the same bits (the row slots' images outlive a launch as well).

What the module found on the MI355X (256 CUs: S = 2048 for the 1000-sample programs, 1024 for the 8192-sample team program):

  * assertion 2 holds in every case, and every probe row and every round-3 row meets the oracle: no output remembers the row before it;
  * fixed with it: pole_zero raised "NaN in output" for a row whose LAST sample is infinite when the last chunk is partial (200 and 1000
    samples, not 1024) -- the recurrence ran on as inf - inf through the pads; double_pole_zero made the whole row NaN the same way;
    min_max_norm with an infinite bound made the whole row NaN where the reference has NaN in the infinite samples alone;
  * fixed with it: fixed_time_pickoff mode 's' of a row with -inf in its last sample.  The reference sweeps the whole row for the
    spline's second derivatives and returns NaN; the device rebuilt them from 48 samples around the pick-off time and returned the
    finite value (programs 1 and 6, all 228 / 114 such rows).  It now looks for a non-finite sample in the row first;
  * fixed with it: the asym_trap_filter reductions (t_lo, t_hi, a_lo, a_hi, tp_0) of the +-3e38 row in program 5.  The reference rounds
    w[i] - w[i - k] to float32, which overflows to an infinity and makes inf - inf a few samples on: NaN; the device's replay from
    speculative carries returned numbers (a_hi +inf).  A replay that leaves the finite numbers is now run again from the true carries,
    as rows with an infinite sample always were.

With a scratch library without the per-row `cx.nan_all = cx.nan_some = 0`, program 1 at 1000 samples gave the same result as the
product library (assertion 2 held): every op that writes a slot also writes its flag before anything reads it, in all six programs."""
import numpy as np
import pytest

import vm_row_loop_cases as V
from test_gpu_processors import DPZ_TOL_F64, FILTER_TOL, FILTER_TOL_F64

pytestmark = pytest.mark.gpu
CASES = V.cases()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    """bit for bit, except that a NaN equals any NaN (and nothing else)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return _bits(a) == _bits(b)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _rows_of(mask):
    return np.flatnonzero(mask.reshape(len(mask), -1).any(axis=1))[:8].tolist()


def _tol(case, kind):
    if case.ft == np.float32:
        return FILTER_TOL
    return DPZ_TOL_F64 if kind == "dpz" else FILTER_TOL_F64


def _kinds(idx, mask):
    """which distinct rows the rows of ``mask`` are: probes by number, poison rows by kind"""
    rows = np.flatnonzero(mask.reshape(len(mask), -1).any(axis=1))
    return [int(u) if u < V.N_PROBES else V.POISON[u - V.N_PROBES] for u in np.unique(idx[rows])]


def _hold(case, name, got, want, bar, idx):
    """one output of every row against the oracle's (``want``: per distinct row; ``idx``: row -> distinct row); returns what differs"""
    ref = np.asarray(want)[idx].astype(got.dtype)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    found = []
    for what, test in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        differ = test(got) != test(ref)
        if differ.any():
            found.append(f"{name}: {what} positions differ in rows {_rows_of(differ)} (distinct rows: {_kinds(idx, differ)})")
    ok = np.isfinite(ref) & np.isfinite(got)
    if bar == "exact":
        bad = ok & (got != ref)
        print(f"{case.name} {name}: exact, {int(bad.sum())} of {int(ok.sum())} finite values differ")
        if bad.any():
            found.append(f"{name}: not bit-exact in rows {_rows_of(bad)} (distinct rows: {_kinds(idx, bad)})")
        return found
    dev = np.abs(np.where(ok, got, 0).astype(np.float64) - np.where(ok, ref, 0).astype(np.float64))
    if bar[0] == "peak":
        rows = np.asarray(bar[1]).astype(np.float64)
        peak = np.max(np.where(np.isfinite(rows), np.abs(rows), 0.0).reshape(len(rows), -1), axis=1)[idx]
        allowed = (_tol(case, bar[2]) * peak).reshape((-1,) + (1,) * (got.ndim - 1))
        scaled = dev / np.where(peak > 0, peak, 1.0).reshape(allowed.shape)
        print(f"{case.name} {name}: worst |dev| / peak {scaled.max():.2e} (bar {_tol(case, bar[2]):g})")
    else:  # ("close", rtol, atol per distinct row): numpy.isclose
        allowed = (bar[2][idx] + bar[1] * np.abs(np.where(ok, ref, 0).astype(np.float64))).reshape(dev.shape)
        print(f"{case.name} {name}: worst |dev| - allowed {np.max(dev - allowed):.2e}")
    bad = ok & (dev > allowed)
    if bad.any():
        found.append(f"{name}: off the bar in rows {_rows_of(bad)} (distinct rows: {_kinds(idx, bad)}), worst excess {float(np.max(dev - allowed)):.3e}")
    return found


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_rows_that_follow_another_on_their_wavefront(case):
    from dspeed_amd.chain import plan
    from dspeed_amd.device import DeviceArray

    with V.switches(case.env):
        chain, small = case.build()
        chain._ensure()
        assert chain._chain.kernel_name.startswith("dsp_vm_kernel"), chain._chain.kernel_name
        assert plan(chain.program, case.ft)["team"] == case.team
        S = V.rows_per_round(chain.geometry(1 << 22), case.team)
        idx = V.layout(S)
        n = len(idx)
        # 1. the launch of these n rows has S row slots: row r + S follows row r on its wavefront(s)
        g = chain.geometry(n)
        assert g["blocks"] * g["waves_per_block"] == S * case.team and n == 3 * S + S // 2 and S >= 2 * V.N_PROBES, (g, S, n)
        table = case.table()
        d_in = case.linked({k: DeviceArray.from_numpy(np.ascontiguousarray(v[idx])) for k, v in table.items()})
        d_out = {k: DeviceArray((n,) + v.shape[1:], v.dtype) for k, v in small.items()}
        chain.link(d_in, d_out)
        chain.execute()  # (every column on the device: one launch over the n rows; a DSPFatal of any row is raised here)
        got = {k: d.to_numpy() for k, d in d_out.items()}
        again = None
        if case.program == 5:
            chain.execute()
            again = {k: d.to_numpy() for k, d in d_out.items()}
    print(f"{case.name}: {n} rows on {S} row slots ({g})")
    want = case.want()
    assert set(got) == set(want)
    # 2. no memory of the previous row: round 2 repeats round 0
    assert np.array_equal(idx[:S], idx[2 * S:3 * S]) and (idx[S:2 * S] >= V.N_PROBES).all() and (idx[3 * S:] != idx[:S // 2]).all()
    for k, v in got.items():
        same = _same_bits(v[:S], v[2 * S:3 * S])
        assert same.all(), (case.name, k, "round 2 differs from round 0 on row slots", _rows_of(~same), "of", int((~same).reshape(S, -1).any(axis=1).sum()))
    # 3. every row against the oracle
    found = [f for k, (ref, bar) in want.items() for f in _hold(case, k, got[k], ref, bar, idx)]
    for f in found:
        print(f"{case.name} DIFFERS {f}")
    assert not found, (case.name, found)
    # 4. the same handle again
    if again is not None:
        for k, v in got.items():
            assert _same_bits(v, again[k]).all(), (case.name, k, "second launch")
