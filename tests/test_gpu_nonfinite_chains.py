"""Filter chains over rows with infinite samples, on the GPU, against the oracle composed processor by processor.

The reference's waveform processors return NaN for a waveform with a NaN anywhere in it, and a recursive filter makes NaNs of its own
from an infinite sample: the inf enters the running value and leaves it L samples later, inf - inf.  Every chain below is run three
ways -- as planned, on the VM with the trapezoid fused into its reductions, and on the VM with the filtered waveform also an output --
and each output is compared with the oracle: indices and pick-offs bit for bit, NaN / inf patterns sample for sample, finite filter
values within 1e-6 of the row's peak."""
import os

import numpy as np
import pytest

import oracle
from dspeed_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 1e-6
M = "dspeed.processors"
MM = ["t_min", "t_max", "a_min", "a_max"]


def _run(recipe, tb, vm=False, env=None):
    from dspeed_amd.processing_chain import build_processing_chain

    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        chain, _, out = build_processing_chain(recipe, tb)
        if vm:
            chain._ensure()
            chain._chain.set_fused(0)
        chain.execute()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return chain, out


def _rows(n, dtype, rise, n_rows, seed, base=100.0):
    """Pulses with infinities at the places where the kernels branch: sample 0, the middle, within `rise` of the end, the last sample,
    both sides of chunk boundaries k C - 1 / k C, two of one sign in a Haar pair, both signs within one window; one all-inf row; clean rows
    (the rest) in between.  Integer rows stay clean.  `base`: the pulses' baseline."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)[None, :]
    t0 = np.floor(rng.uniform(0.3, 0.5, (n_rows, 1)) * n)
    x = base + rng.uniform(200, 2000, (n_rows, 1)) * np.exp(-(i - t0) / 1716.28) * (i >= t0) + 5 * rng.standard_normal((n_rows, n))
    if np.dtype(dtype).kind == "i":
        return np.round(x).astype(dtype)
    w = x.astype(dtype)
    C = -(-n // 64)
    places = [[(0, 1)], [(n // 2, 1)], [(n - rise // 2, 1)], [(n - 1, -1)], [(5 * C - 1, 1)], [(5 * C, -1)], [(n // 2, 1), (n // 2 + 1, 1)],
              [(n // 3, 1), (n // 3 + rise // 2, -1)], [(3 * C, -1), (n - 2, -1)]]
    for r, pl in enumerate(places):
        for at, sgn in pl:
            w[2 * r + 1, at] = sgn * np.inf  # (even rows clean)
    w[2 * len(places) + 1, :] = np.inf
    return w


def _same_nonfinite(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:8])
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (what, np.argwhere(np.isposinf(got) != np.isposinf(want))[:8])
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, np.argwhere(np.isneginf(got) != np.isneginf(want))[:8])


def _close(got, want, peak, what, tol=TOL):
    """NaN / inf patterns equal; finite values within tol of the row's peak (the filtered row's largest finite magnitude)"""
    _same_nonfinite(got, want, what)
    ok = np.isfinite(want)
    bar = tol * np.broadcast_to(peak.reshape((-1,) + (1,) * (want.ndim - 1)), want.shape)
    dev = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(dev[ok] <= bar[ok]), (what, float(np.max(dev[ok] - bar[ok])))


def _peak(f):
    a = np.where(np.isfinite(f), np.abs(f.astype(np.float64)), 0.0)
    return np.maximum(a.max(axis=1), 1.0)


def _trap_cases():
    """(name, processor call, oracle of the filtered row, the readers wanted)"""
    return [
        ("trap_filter", "trap_filter(waveform, 40, 12, wf_t)", lambda w: oracle.trap_filter(w, 40, 12)[0], "min_max+tpt"),
        ("trap_norm", "trap_norm(waveform, 40, 12, wf_t)", lambda w: oracle.trap_norm(w, 40, 12)[0], "amax"),
        ("asym_trap", "asym_trap_filter(waveform, 8, 4, 125, wf_t)", lambda w: oracle.asym_trap_filter(w, 8, 4, 125)[0], "tpt_fwd"),
        ("trap_pickoff", "trap_filter(waveform, 40, 12, wf_t)", lambda w: oracle.trap_filter(w, 40, 12)[0], "pickoff"),
    ]


def _recipe(call, red, with_wf):
    procs = {"wf_t": f"{M}.{call}"}
    outs = []
    if red in ("min_max+tpt",):
        procs["t_min, t_max, a_min, a_max"] = {"function": "min_max", "module": M, "args": ["wf_t", *MM]}
        procs["tp_b"] = f"{M}.time_point_thresh(wf_t, thr, t_max, 0, tp_b)"
        outs = MM + ["tp_b"]
    elif red == "amax":
        procs["a_max"] = {"function": "amax", "module": "numpy", "args": ["wf_t", 1, "a_max"]}
        outs = ["a_max"]
    elif red == "tpt_fwd":
        procs["tp_f"] = f"{M}.time_point_thresh(wf_t, thr, 3, 1, tp_f)"
        outs = ["tp_f"]
    else:
        procs["e_l"] = {"function": "fixed_time_pickoff", "module": M, "args": ["wf_t", "t_pick", "'l'", "e_l"]}
        procs["e_n"] = {"function": "fixed_time_pickoff", "module": M, "args": ["wf_t", "t_pick", "'n'", "e_n"]}
        outs = ["e_l", "e_n"]
    return {"outputs": outs + (["wf_t"] if with_wf else []), "processors": procs}


def _want(red, f, tb):
    if red == "min_max+tpt":
        tmin, tmax, amin, amax, _ = oracle.min_max(f)
        tp = oracle.time_point_thresh(f, tb["thr"], tmax, 0)[0]
        return {"t_min": tmin, "t_max": tmax, "a_min": amin, "a_max": amax, "tp_b": tp}
    if red == "amax":
        return {"a_max": np.max(f, axis=1)}  # (numpy.amax: NaN wins)
    if red == "tpt_fwd":
        return {"tp_f": oracle.time_point_thresh(f, tb["thr"], np.full(len(f), 3, f.dtype), 1)[0]}
    return {"e_l": oracle.fixed_time_pickoff(f, tb["t_pick"], "l")[0], "e_n": oracle.fixed_time_pickoff(f, tb["t_pick"], "n")[0]}


def _check(out, want, f, what):
    peak = _peak(f)
    for k, v in want.items():
        got = np.asarray(out[k])
        if k.startswith("t_") or k.startswith("tp"):
            assert np.array_equal(got, v, equal_nan=True), (what, k, np.argwhere(~((got == v) | (np.isnan(got) & np.isnan(v))))[:8].ravel())
        else:
            _close(got, v.astype(got.dtype), peak, f"{what} {k}")


# 8192 = 64 x 128 fills its chunks (the full-row maximum form); the others do not.  Row counts off any workgroup multiple.
LENGTHS = [(8192, 75), (4096, 37), (3000, 21), (1000, 37)]
SHAPES = [(np.float32, n, r) for n, r in LENGTHS] + [(np.float64, 8192, 75), (np.float64, 1000, 37)] + [(np.int16, n, r) for n, r in LENGTHS]


@pytest.mark.parametrize("dtype,n,n_rows", SHAPES, ids=lambda v: getattr(v, "__name__", str(v)))
@pytest.mark.parametrize("case", _trap_cases(), ids=lambda c: c[0])
def test_trapezoid_chains_with_infinities(case, dtype, n, n_rows):
    name, call, filt, red = case
    w = _rows(n, dtype, 40 if "asym" not in name else 125, n_rows, seed=n + len(name))
    ft = np.float64 if dtype is np.float64 else np.float32
    rng = np.random.default_rng(n)
    tb = {"waveform": w, "thr": rng.uniform(50, 2000, n_rows).astype(ft),
          "t_pick": np.floor(rng.uniform(0, n - 1, n_rows)).astype(ft) + ft(0.25)}
    f = filt(w.astype(ft))
    want = _want(red, f, tb)
    planned, p_out = _run(_recipe(call, red, False), tb)
    kinds = [k for _w, k in planned.kernels()]
    assert kinds, planned.kernels()
    _check(p_out, want, f, f"{name} planned {kinds}")
    fused, v_out = _run(_recipe(call, red, False), tb, vm=True)
    ops = [o[0] for o in fused.program.ops]
    if red != "pickoff":
        assert _lib.OP_TRAP_REDUCE in ops, ops
    _check(v_out, want, f, f"{name} VM fused")
    _, s_out = _run(_recipe(call, red, True), tb, vm=True)
    _check(s_out, want, f, f"{name} VM stored")
    _close(np.asarray(s_out["wf_t"]), f.astype(np.asarray(s_out["wf_t"]).dtype), _peak(f), f"{name} VM stored wf_t")
    if np.dtype(dtype).kind == "i":
        assert np.all(np.isfinite(f))
    else:
        assert np.isnan(f[1, -1]) and not np.isnan(f[0]).any()  # (the table does reach the NaN case)


@pytest.mark.parametrize("n,n_rows", [(4784, 37), (1000, 21)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moving_windows_with_infinities(dtype, n, n_rows):
    w = _rows(n, dtype, 48, n_rows, seed=5 * n, base=0.0)  # (a current-like row: no pedestal under the pulse)
    rec = {"outputs": MM + ["wf_mw"], "processors": {
        "wf_mw": f"{M}.moving_window_multi(waveform, 48, 3, 0, wf_mw)",
        "t_min, t_max, a_min, a_max": {"function": "min_max", "module": M, "args": ["wf_mw", *MM]}}}
    f = oracle.moving_window_multi(w, 48, 3, 0)[0]
    tmin, tmax, amin, amax, _ = oracle.min_max(f)
    want = {"t_min": tmin, "t_max": tmax, "a_min": amin, "a_max": amax}
    for env in ({}, {"DSPEED_HIP_NO_TEAMS": "1"}):
        for vm in (False, True):
            _, out = _run(rec, {"waveform": w}, vm=vm, env=env)
            _check(out, want, f, f"moving_window_multi vm={vm} {env}")
            # (stored samples: the float32 scan over three 4784-sample passes drifts to 1.3e-6 of the peak on clean rows -- the finite path,
            # which infinities do not touch; the per-event values above keep the 1e-6 bar)
            wf_tol = 2 * TOL if dtype is np.float32 and n > 4096 else TOL
            _close(np.asarray(out["wf_mw"]), f, _peak(f), f"moving_window_multi wf vm={vm} {env}", wf_tol)
    assert np.isnan(f[1]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_haar_dwt_with_infinities(dtype):
    n, n_rows = 8192, 37
    w = _rows(n, dtype, 40, n_rows, seed=91)
    rec = {"outputs": MM + ["wf_d"], "processors": {
        "wf_d": {"function": "discrete_wavelet_transform", "module": M, "args": ["waveform", 5, "'h'", "'a'", "wf_d(256, 'f')"]},
        "t_min, t_max, a_min, a_max": {"function": "min_max", "module": M, "args": ["wf_d", *MM]}}}
    f = oracle.dwt_haar(w, 5, "a", 256)[0]
    tmin, tmax, amin, amax, _ = oracle.min_max(f)
    want = {"t_min": tmin, "t_max": tmax, "a_min": amin, "a_max": amax}
    for vm in (False, True):
        _, out = _run(rec, {"waveform": w}, vm=vm)
        _check(out, want, f, f"dwt vm={vm}")
        _close(np.asarray(out["wf_d"]), f, _peak(f), f"dwt wf vm={vm}")
    assert np.isnan(f).any(axis=1).sum() >= 1  # (the +inf, -inf window meets in one level's pair)
