"""Do the cases of lane_kernel_cases.py say something?  On the oracle alone (and the planner, which needs no device): every oracle call
succeeds, the rows make the outputs vary -- a comparison of NaN with NaN, or of one index seventy times, would pass whatever the kernel
did -- the scaled rows reach the denormals and the overflow they are there for, and every case is planned onto the kernel its table names.
If a changed generator breaks a condition here, the generator is what changes."""
import numpy as np
import pytest

import lane_kernel_cases as K

CURRENT_ALL = [K.CURRENT_DEFAULT] + K.CURRENT_TIGHT + K.CURRENT_SMALL


def _planned_kernel(recipe, tb, promise=False):
    from dspeed_amd.chain import plan
    from dspeed_amd.processing_chain import build_processing_chain

    chain, _, _ = build_processing_chain(recipe, tb)
    assert not chain._stages and chain._tail is None and chain._walks is None  # (one program, one kernel)
    if promise:
        K.set_load_promise(chain.program)
    return plan(chain.program)["kernel"]


def test_generators_are_deterministic():
    for gen in (lambda: K.current_rows(3)[0], lambda: K.synth_rows(4)[0], lambda: K.thresholds(5), lambda: K.fit_rows(70, 100, np.int16, 6),
                lambda: K.current_starts(7, K.current_rows(3)[1], 1024, 301)):
        assert np.array_equal(gen(), gen(), equal_nan=True)


@pytest.mark.parametrize("p", CURRENT_ALL, ids=K.current_id)
def test_current_branch_configurations_vary(p):
    wf, t0 = K.current_rows(sum(p.values()))
    start = K.current_starts(1, t0, 1024, p["n_win"], special=False)
    want = K.current_oracle(wf, start, p)
    assert not np.isnan(want["a_hi"]).any() and not np.isnan(want["t_hi"]).any()
    assert len(np.unique(want["t_hi"])) >= 3, np.unique(want["t_hi"])
    assert _planned_kernel(K.current_recipe(p), {"wf": wf, "t_start": start}) == "dsp_current_kernel"
    # the special starts: NaN rows exactly where the window does not exist
    start = K.current_starts(1, t0, 1024, p["n_win"])
    a_hi = K.current_oracle(wf, start, p)["a_hi"]
    for row, exists in K.CURRENT_SPECIAL_STARTS.items():
        assert np.isnan(a_hi[row]) == (not exists), row


@pytest.mark.parametrize("p", K.CURRENT_TIGHT, ids=K.current_id)
def test_current_branch_refused_neighbours_are_the_vm_s(p):
    """one sample less of window: the last upsampled sample has no current sample behind it.  The oracle's answer is NaN throughout (the
    upsampler leaves that sample NaN); a kernel that took the shape would read a checkpoint there and return plausible numbers"""
    q = K.current_refused(p)
    wf, t0 = K.current_rows(sum(q.values()))
    start = K.current_starts(1, t0, 1024, q["n_win"], special=False)
    assert ((q["n_up"] - 1 + q["up"] // 2) // q["up"]) == q["n_win"] - q["ac"]  # exactly one past the limit
    assert np.isnan(K.current_oracle(wf, start, q)["a_hi"]).all()
    assert _planned_kernel(K.current_recipe(q), {"wf": wf, "t_start": start}).startswith("dsp_vm")


def test_current_branch_scaled_rows_reach_denormals_and_overflow():
    p = K.CURRENT_DEFAULT
    wf, t0 = K.current_rows(sum(p.values()))
    start = K.current_starts(1, t0, 1024, p["n_win"], special=False)
    tiny = np.float32(np.finfo(np.float32).tiny)
    a = K.current_oracle(K.scaled(wf, 1e-42), start, p)["a_hi"]
    assert np.all((a != 0) & (np.abs(a) < tiny))          # every maximum a non-zero denormal
    a = K.current_oracle(K.scaled(wf, 1e30), start, p)["a_hi"]
    assert np.isfinite(a).all()
    a = K.current_oracle(K.scaled(wf, 3e34), start, p)["a_hi"]
    assert 0 < np.isnan(a).sum() < len(a)                 # rows that overflow (inf - inf) beside rows that do not


@pytest.mark.parametrize("p", [K.CURRENT_DEFAULT] + K.CURRENT_TIGHT, ids=K.current_id)
def test_current_branch_promise_is_planned(p):
    wf, t0 = K.current_rows(9)
    tb = {"wf": wf, "t_start": K.current_starts(1, t0, 1024, p["n_win"])}
    assert _planned_kernel(K.current_recipe(p), tb, promise=True) == "dsp_current_kernel"


@pytest.mark.parametrize("c", K.ROWS_ALL, ids=lambda c: c["name"])
def test_rows_kernel_cases_find_crossings(c):
    recipe, tb, want = K.rows_case(c)
    assert np.isfinite(want["tp_0"]).sum() * 4 >= K.N_ROWS, np.isfinite(want["tp_0"]).sum()
    assert len(np.unique(want["tp_max"][~np.isnan(want["tp_max"])])) >= 3
    assert _planned_kernel(recipe, tb).startswith(c["kernel"])
    if c["bl"] == "nan_in_row_9":
        assert np.flatnonzero(np.isnan(want["wf_max"])).tolist() == [9]
    if c["scale"] == 1e-42:
        x = np.abs(tb["waveform"])  # (more than half of the samples are non-zero denormals, and so is every threshold)
        assert np.count_nonzero((x > 0) & (x < np.finfo(np.float32).tiny)) > x.size // 2 and np.all((tb["thr"] > 0) & (tb["thr"] < 1e-40))
    if c["scale"] == 1e30:
        assert np.isfinite(want["wf_max"]).all() and want["wf_max"].max() > 1e32


@pytest.mark.parametrize("walk", list(K.ROWS_WALKS))
@pytest.mark.parametrize("trap", K.ROWS_TRAPS, ids=lambda t: "-".join(map(str, t)))
def test_rows_kernel_consumer_cases_find_crossings(trap, walk):
    recipe, tb, want = K.walk_case(trap, walk)
    assert len(np.unique(want["tp_max"])) >= 3 and not np.isnan(want["wf_max"]).any()
    if K.ROWS_WALKS[walk] is not None:
        assert np.isfinite(want["tp_0"]).sum() * 4 >= K.N_ROWS, np.isfinite(want["tp_0"]).sum()
    assert _planned_kernel(recipe, tb) == "dsp_rows_kernel"


@pytest.mark.parametrize("dtype,trap", K.STOP_CASES, ids=lambda v: np.dtype(v).name if isinstance(v, type) else "-".join(map(str, v)))
def test_rows_kernel_stop_cases(dtype, trap):
    recipe, tb, tp0 = K.stop_case(dtype, trap)
    ts = tb["ts"]
    assert np.isnan(tp0[64:128]).all() and np.isnan(ts[64:128]).all()               # a group without a valid start
    assert ts[128:192].max() == ts[130] == tb["waveform"].shape[1] - 1              # a group that walks to the last block
    assert np.isnan(tp0[4]) and (dtype is not np.float32 or np.isnan(tp0[K.STOP_NAN_ROW]))  # a NaN start, a NaN row
    for group in (slice(0, 64), slice(128, 192), slice(192, 200)):
        assert np.isfinite(tp0[group]).sum() * 4 >= len(tp0[group])
    assert _planned_kernel(recipe, tb, promise=True) == "dsp_rows_kernel"


def test_fit_windows_of_one_and_two_samples_on_the_oracle():
    import oracle

    w = K.fit_rows(70, 100, np.float32, 1)
    *_o, rc = oracle.linear_slope_fit(np.ascontiguousarray(w[:, 10:11]))
    assert rc != 0  # one sample: the reference raises ZeroDivisionError
    got = K.fit_oracle(w, [(0, 10, 2)], None, 0, None, np.float32)
    assert np.isfinite(got).all() and len(np.unique(got[0, 2])) > 3


def test_fit_rows_entry_point_refuses_a_window_of_one_sample():
    """dsp_linear_slope_fit_rows checks its windows before it touches the device: DSP_E_ZERODIV with the in-chain op's message, wherever
    the window stands among the fits (the pointers are never followed: the call returns first)"""
    from dspeed_amd import _lib
    from dspeed_amd.device import dtype_code

    rows, out = np.zeros((7, 100), np.float32), np.zeros((8, 7), np.float32)
    f32 = dtype_code(np.float32)
    for fits in ([(0, 10, 1)], [(0, 10, 20), (0, 99, 1)]):
        win = (_lib.FitWindow * len(fits))(*[_lib.FitWindow(*f) for f in fits])
        rc = _lib.lib().dsp_linear_slope_fit_rows(rows.ctypes.data, f32, 7, 100, 100, f32, None, 0, 0.0, 0, 0, 0.0, win, len(fits), out.ctypes.data, None)
        assert rc == _lib.E_ZERODIV and _lib.last_error() == _lib.fatal_message(_lib.E_ZERODIV) == "division by zero"
        with pytest.raises(ZeroDivisionError):
            _lib.check(rc, what="fit rows")
    assert not out.any()
