"""GPU parity of whole dspeed recipes (JSON -> device program -> one launch) against the oracle run processor by processor,
the way the reference's ProcessingChain does it."""
import numpy as np
import pytest

import oracle
import recipes
from dspeed_amd import _lib as _LIB
from golden_util import assert_rel_to_peak, cases

pytestmark = pytest.mark.gpu
TOL = 1e-6


def _synth(rng, n_wf, wf_len, bl=(9000, 11000), amp=(500, 15000)):
    i = np.arange(wf_len, dtype=np.float64)[None, :]
    B = rng.uniform(*bl, (n_wf, 1))
    A = rng.uniform(*amp, (n_wf, 1))
    t0 = np.floor(rng.uniform(0.45, 0.55, (n_wf, 1)) * wf_len)
    x = B + A * np.exp(-(i - t0) / 1716.28) * (i >= t0) + 5.0 * rng.standard_normal((n_wf, wf_len))
    return x, B[:, 0].astype(np.float32), t0[:, 0]


def _run(recipe, tb, vm=False, **kw):
    from dspeed_amd.processing_chain import build_processing_chain

    chain, mask, tb_out = build_processing_chain(recipe, tb, **kw)
    if vm:  # the generic waveform VM, whatever specialised kernel the recipe's shape would select
        chain._ensure()
        chain._chain.set_fused(0)
    chain.execute()
    return chain, tb_out


def test_c1_recipe_golden():
    c1 = cases("chains")[0]
    _, out = _run(recipes.C1, {"waveform": c1["waveform"]})
    assert_rel_to_peak(out["wf_trap"], c1["wf_trap"], TOL, "C1 wf_trap")


def test_c2_recipe_golden_and_units_form():
    from dspeed_amd.processing_chain import WaveformInput

    c2 = cases("chains")[1]
    tb = {"waveform": c2["waveform"], "baseline": c2["baseline"], "t_pick": c2["t_pick"]}
    chain, out = _run(recipes.C2, tb)
    want = c2["trapEftp"]
    assert np.array_equal(np.isnan(out["trapEftp"]), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.max(np.abs(out["trapEftp"][ok] - want[ok]) / np.abs(want[ok])) <= TOL
    assert chain._chain.kernel_name.startswith("dsp_energy")  # the recipe took the specialised path
    tb["waveform"] = WaveformInput(c2["waveform"], dt=16.0)
    # the LEGEND-style form: tau = 27460.5 ns / 16 ns (not exactly the 1716.28 of the fixture), rise/flat from time quantities;
    # wf_trap is an output there, so this runs on the generic VM with a materialised trapezoid
    _, out2 = _run(recipes.C2_UNITS, tb)
    want2, rc = oracle.chain_energy(c2["waveform"], c2["baseline"], c2["t_pick"], 27460.5 / 16.0, 625, 188, "l")
    assert rc == 0 and np.array_equal(np.isnan(out2["trapEftp"]), np.isnan(want2))
    assert np.max(np.abs(out2["trapEftp"][ok] - want2[ok]) / np.abs(want2[ok])) <= TOL
    xb = oracle.bl_subtract(c2["waveform"], c2["baseline"])[0]
    tr = oracle.trap_filter(oracle.pole_zero(xb, 27460.5 / 16.0)[0], 625, 188)[0]
    assert_rel_to_peak(out2["wf_trap"], tr, TOL, "wf_trap")


def test_c5_recipe_golden():
    c5 = cases("chains")[2]
    tb = {"waveform": c5["waveform"], "thr": c5["thr"]}
    _, out = _run(recipes.C5, tb)
    mm = c5["min_max"]
    # index results are exact only on identical filter outputs: compare values to tolerance, indices where the
    # device filter output reproduces the reference's
    w = c5["waveform"].astype(np.float32)
    dpz = oracle.double_pole_zero(w, 1716.28, 62.5, 0.02)[0]
    assert_rel_to_peak(out["wf_max"], mm[:, 3], TOL, "wf_max")
    assert_rel_to_peak(out["wf_min"], mm[:, 2], 1e-5, "wf_min")
    assert np.all(np.abs(out["tp_max"] - mm[:, 1]) <= 1) and np.all(np.abs(out["tp_0"] - c5["tp_0"]) <= 1)
    dwt = oracle.dwt_haar(dpz, 5, "a", 256)[0]
    assert_rel_to_peak(out["dwt_haar"], dwt, TOL, "dwt_haar")


def test_c5_stages_bit_exact_on_identical_inputs():
    """min_max / time_point_thresh / dwt fed the reference's own filter output are bit-exact (run through the recipe API)."""
    c5 = cases("chains")[2]
    at = oracle.asym_trap_filter(oracle.double_pole_zero(c5["waveform"].astype(np.float32), 1716.28, 62.5, 0.02)[0], 8, 4, 125)[0]
    r = {"outputs": ["tp_0", "tp_min", "tp_max", "wf_min", "wf_max"], "processors": {
        "tp_min, tp_max, wf_min, wf_max": {"function": "min_max", "module": "dspeed.processors", "args": ["wf", "tp_min", "tp_max", "wf_min", "wf_max"]},
        "tp_0": {"function": "time_point_thresh", "module": "dspeed.processors", "args": ["wf", "thr", "tp_max", 0, "tp_0"]}}}
    _, out = _run(r, {"wf": at, "thr": c5["thr"]})
    mm = c5["min_max"]
    for k, nm in enumerate(("tp_min", "tp_max", "wf_min", "wf_max")):
        assert np.array_equal(out[nm], mm[:, k]), nm
    assert np.array_equal(out["tp_0"], c5["tp_0"])


def test_c3_small_recipe_vs_oracle():
    rng = np.random.default_rng(33)
    x, bl, _ = _synth(rng, 24, 512)
    wf = x.astype(np.float32)
    r = recipes.c3_small(512, 129, 0, 400)
    chain, out = _run(r, {"waveform": wf, "baseline": bl})
    xb = oracle.bl_subtract(wf, bl)[0]
    kz = chain._consts["taps:zac_kernel"][:129]  # (the binding holds zeros after the taps up to a multiple of 16)
    kc = chain._consts["taps:cusp_kernel"][:129]
    want_z = oracle.convolve_wf(xb, kz, "v", 272, in_len=400)[0]
    want_c = oracle.convolve_wf(xb, kc, "v", 272, in_len=400)[0]
    assert_rel_to_peak(out["wf_zac"], want_z, TOL, "wf_zac")
    assert np.max(np.abs(out["zacEmax"] - want_z.max(axis=1)) / np.abs(want_z).max(axis=1)) <= TOL
    assert np.max(np.abs(out["cuspEmax"] - want_c.max(axis=1)) / np.abs(want_c).max(axis=1)) <= TOL


def test_c3_icpc_geometry_golden():
    """5792-tap cusp/zac over wf[:6092] of 8192-sample rows -> 301 outputs (BASELINE configs[2] geometry)"""
    g = {c.name: c for c in cases("convolutions", tag="f32")}
    cz, cc = g["f32_icpc_zac_filter"], g["f32_icpc_cusp_filter"]
    wf = cz["w_in"]  # already baseline subtracted in the fixture: feed baseline 0
    _, out = _run(recipes.C3, {"waveform": wf, "baseline": np.zeros(len(wf), dtype=np.float32)})
    for nm, c in (("zacEmax", cz), ("cuspEmax", cc)):
        want = c["w_out"]
        assert np.max(np.abs(out[nm] - want.max(axis=1)) / np.abs(want).max(axis=1)) <= TOL, nm


def test_chain_executes_in_row_ranges_and_on_device_buffers():
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processing_chain import build_processing_chain

    rng = np.random.default_rng(5)
    x, bl, t0 = _synth(rng, 100, 4096)
    wf = x.astype(np.float32)
    tp = (t0 + 625 + 150.4).astype(np.float32)
    want, _ = oracle.chain_energy(wf, bl, tp, 1716.28, 625, 188, "l")
    chain, mask, tb_out = build_processing_chain(recipes.C2, {"waveform": wf, "baseline": bl, "t_pick": tp})
    chain.execute(0, 37)
    chain.execute(37, 100)
    assert np.max(np.abs(tb_out["trapEftp"] - want) / np.abs(want)) <= TOL
    full = tb_out["trapEftp"].copy()
    # device-resident I/O: nothing crosses PCIe in execute()
    tb_dev = {"waveform": DeviceArray.from_numpy(wf), "baseline": DeviceArray.from_numpy(bl), "t_pick": DeviceArray.from_numpy(tp)}
    out_dev = {"trapEftp": DeviceArray((100,), np.float32)}
    chain(tb_dev, out_dev)
    assert np.array_equal(out_dev["trapEftp"].to_numpy(), full)


def test_energy_recipe_variants_take_the_specialised_kernel():
    """the shapes the specialised kernel accepts besides BASELINE's: constant baseline and pick-off time, no bl_subtract at all,
    trap_norm and asym_trap_filter as the shaping filter, time quantities; each against the oracle run processor by processor"""
    rng = np.random.default_rng(21)
    x, bl, t0 = _synth(rng, 130, 4096, bl=(9999.5, 10000.5))
    wf = x.astype(np.float32)
    M = "dspeed.processors"

    def run(procs, tb, out="e"):
        chain, o = _run({"outputs": [out], "processors": procs}, tb)
        assert chain._chain.kernel_name == "dsp_energy_rr_kernel", chain._chain.kernel_name
        return o[out]

    peak = lambda tr: np.max(np.abs(tr), axis=1)  # noqa: E731
    # constant baseline, constant pick-off time
    got = run({"b": f"{M}.bl_subtract(waveform, 10000, b)", "p": f"{M}.pole_zero(b, 1716.28, p)", "t": f"{M}.trap_filter(p, 400, 100, t)",
               "e": f"{M}.fixed_time_pickoff(t, 2900.25, 'l', e)"}, {"waveform": wf})
    pz = oracle.pole_zero(oracle.bl_subtract(wf, np.float32(10000))[0], 1716.28)[0]
    tr = oracle.trap_filter(pz, 400, 100)[0]
    want = oracle.fixed_time_pickoff(tr, np.float32(2900.25), "l")[0]
    assert np.max(np.abs(got - want) / peak(tr)) <= TOL
    # no bl_subtract: pole_zero straight on the input
    got = run({"p": f"{M}.pole_zero(waveform, 1716.28, p)", "t": f"{M}.trap_filter(p, 200, 50, t)",
               "e": f"{M}.fixed_time_pickoff(t, t_pick, 'n', e)"}, {"waveform": wf, "t_pick": (t0 + 300.7).astype(np.float32)})
    pz = oracle.pole_zero(wf, 1716.28)[0]
    tr = oracle.trap_filter(pz, 200, 50)[0]
    want = oracle.fixed_time_pickoff(tr, (t0 + 300.7).astype(np.float32), "n")[0]
    assert np.max(np.abs(got - want) / peak(tr)) <= TOL
    # trap_norm and asym_trap_filter, per-event baseline, Hermite pick-off
    for name, args, ref in (("trap_norm", "300, 80", lambda p: oracle.trap_norm(p, 300, 80)[0]),
                            ("asym_trap_filter", "100, 40, 300", lambda p: oracle.asym_trap_filter(p, 100, 40, 300)[0])):
        got = run({"b": f"{M}.bl_subtract(waveform, baseline, b)", "p": f"{M}.pole_zero(b, 1716.28, p)", "t": f"{M}.{name}(p, {args}, t)",
                   "e": f"{M}.fixed_time_pickoff(t, t_pick, 'h', e)"}, {"waveform": wf, "baseline": bl, "t_pick": (t0 + 350.3).astype(np.float32)})
        pz = oracle.pole_zero(oracle.bl_subtract(wf, bl)[0], 1716.28)[0]
        tr = ref(pz)
        want = oracle.fixed_time_pickoff(tr, (t0 + 350.3).astype(np.float32), "h")[0]
        assert np.max(np.abs(got - want) / peak(tr)) <= TOL, name


@pytest.mark.parametrize("trap,targs", [("asym_trap_filter", "8, 4, 125"), ("trap_filter", "100, 30"), ("trap_norm", "64, 16")])
def test_trapezoid_fused_with_its_reductions_equals_the_unfused_ops(trap, targs):
    """a trapezoid that only feeds min_max / time_point_thresh is never stored (TRAP_REDUCE): on the waveform VM the same numbers as the
    three ops run one after the other -- forward and backward walks, per-event thresholds, start from t_max / t_min / a column, NaN rows,
    DSPFatal.  (Behind a pole-zero stage the shape belongs to the lane-per-waveform kernel, which is bit-exact against the oracle:
    tests/test_gpu_rows_kernel.py; here the VM's fused op is checked against the VM's own unfused ops.)"""
    from dspeed_amd.errors import DSPFatal

    rng = np.random.default_rng(77)
    x, bl, t0 = _synth(rng, 150, 4096, bl=(-50, 50))
    wf = x.astype(np.float32)
    wf[9, 100] = np.nan
    thr = rng.uniform(5, 400, 150).astype(np.float32)
    thr[11] = np.nan
    start = np.floor(rng.uniform(0, 4095, 150)).astype(np.float32)
    M = "dspeed.processors"
    mm = {"function": "min_max", "module": M, "args": ["wf_t", "t_min", "t_max", "a_min", "a_max"]}

    def recipe(outs, tpt_args):
        procs = {"wf_pz": f"{M}.pole_zero(waveform, 1716.28, wf_pz)", "wf_t": f"{M}.{trap}(wf_pz, {targs}, wf_t)",
                 "t_min, t_max, a_min, a_max": mm}
        for name, a in tpt_args.items():
            procs[name] = f"{M}.time_point_thresh(wf_t, {a}, {name})"
        return {"outputs": outs, "processors": procs}

    tb = {"waveform": wf, "thr": thr, "start": start}
    tpts = {"tp_b": "thr, t_max, 0", "tp_f": "thr, start, 1"}
    for use in ({"tp_b": tpts["tp_b"]}, {"tp_f": tpts["tp_f"]}, {}):
        names = ["t_min", "t_max", "a_min", "a_max", *use]
        fused_chain, fused = _run(recipe(names, use), tb, vm=True)
        plain_chain, plain = _run(recipe(names + ["wf_t"], use), tb)
        from dspeed_amd import _lib

        f_ops = [o[0] for o in fused_chain.program.ops]
        assert _lib.OP_TRAP_REDUCE in f_ops and _lib.OP_MIN_MAX not in f_ops
        assert _lib.OP_TRAP_REDUCE not in [o[0] for o in plain_chain.program.ops]
        for nm in names:
            assert np.array_equal(fused[nm], plain[nm], equal_nan=True), (trap, nm)
        assert np.isnan(fused["a_max"][9]) and (not use or np.isnan(fused[next(iter(use))][11]))
    # time_point_thresh alone (no min_max), and its data-dependent DSPFatal with the absolute row
    only = {"outputs": ["tp"], "processors": {"wf_t": f"{M}.{trap}(waveform, {targs}, wf_t)", "tp": f"{M}.time_point_thresh(wf_t, thr, start, 0, tp)"}}
    c1, o1 = _run(only, tb)
    assert [o[0] for o in c1.program.ops].count(_lib.OP_TRAP_REDUCE) == 1
    only2 = {"outputs": ["tp", "wf_t"], "processors": dict(only["processors"])}
    _, o2 = _run(only2, tb)
    assert np.array_equal(o1["tp"], o2["tp"], equal_nan=True)
    bad = start.copy()
    bad[40] = 17.5
    from dspeed_amd.processing_chain import build_processing_chain

    cb, _, _ = build_processing_chain(only, {"waveform": wf, "thr": thr, "start": bad})
    with pytest.raises(DSPFatal, match="starting index must be an integer") as ei:
        cb.execute()
    assert ei.value.wf_range == range(40, 41)


def test_baseline_statistics_feed_thresholds_like_the_icpc_recipe():
    """icpc-dsp-config.json:45-69, 294-305: linear_slope_fit on the baseline slice gives bl_std, which scales the threshold of the t0
    search on the asymmetric trapezoid; per-event expression (bl_std * 4), slice of an intermediate, the fused trapezoid reductions"""
    rng = np.random.default_rng(71)
    x, bl, t0 = _synth(rng, 60, 4096)
    wf = x.astype(np.float32)
    M = "dspeed.processors"
    rec = {"outputs": ["bl_mean", "bl_std", "bl_slope", "tp_0"], "processors": {
        "wf_blsub": f"{M}.bl_subtract(waveform, baseline, wf_blsub)",
        "bl_mean, bl_std, bl_slope, bl_intercept": {"function": "linear_slope_fit", "module": M,
                                                     "args": ["wf_blsub[0:750]", "bl_mean", "bl_std", "bl_slope", "bl_intercept"]},
        "wf_pz": f"{M}.pole_zero(wf_blsub, 1716.28, wf_pz)",
        "wf_atrap": f"{M}.asym_trap_filter(wf_pz, 8, 4, 125, wf_atrap)",
        "tp_min, tp_max, wf_min, wf_max": {"function": "min_max", "module": M, "args": ["wf_atrap", "tp_min", "tp_max", "wf_min", "wf_max"]},
        "tp_0": f"{M}.time_point_thresh(wf_atrap, bl_std*4, tp_max, 0, tp_0)"}}
    _, out = _run(rec, {"waveform": wf, "baseline": bl})
    xb = oracle.bl_subtract(wf, bl)[0]
    mean, std, slope, icpt, rc = oracle.linear_slope_fit(np.ascontiguousarray(xb[:, :750]))
    assert rc == 0
    assert np.array_equal(out["bl_mean"], mean) and np.array_equal(out["bl_std"], std)
    assert np.max(np.abs(out["bl_slope"] - slope)) <= 1e-7
    at = oracle.asym_trap_filter(oracle.pole_zero(xb, 1716.28)[0], 8, 4, 125)[0]
    tmin, tmax, amin, amax, _ = oracle.min_max(at)
    tp0 = oracle.time_point_thresh(at, (std * np.float32(4)).astype(np.float32), tmax, 0)[0]
    assert np.all(np.abs(out["tp_0"] - tp0) <= 1)


def test_current_branch_of_the_icpc_recipe():
    """the A/E branch as the production recipe writes it (icpc-dsp-config.json:306-346): windower -> avg_current -> upsampler ->
    moving_window_multi -> min_max -> numpy.add, one device program, against the oracle run processor by processor"""
    rng = np.random.default_rng(61)
    x, bl, t0 = _synth(rng, 80, 4096)
    wf = x.astype(np.float32)
    est = (t0 - 100).astype(np.float32)
    M = "dspeed.processors"
    rec = {"outputs": ["A_max", "tp_aoe_samp"], "processors": {
        "wf_pz": f"{M}.pole_zero(waveform, 1716.28, wf_pz)",
        "wf_le": f"{M}.windower(wf_pz, tp_0_est, wf_le(301, 'f'))",
        "curr": f"{M}.avg_current(wf_le, 1, curr(300, 'f'))",
        "curr_up": f"{M}.upsampler(curr, 16, curr_up(4784, 'f'))",
        "curr_av": f"{M}.moving_window_multi(curr_up, 48, 3, 0, curr_av)",
        "aoe_t_min, tp_aoe_max, A_min, A_max": {"function": "min_max", "module": M, "args": ["curr_av", "aoe_t_min", "tp_aoe_max", "A_min", "A_max"]},
        "tp_aoe_samp": {"function": "add", "module": "numpy", "args": ["tp_0_est", "tp_aoe_max/16", "tp_aoe_samp"]}}}
    _, out = _run(rec, {"waveform": wf, "tp_0_est": est})
    pz = oracle.pole_zero(wf, 1716.28)[0]
    le = oracle.windower(pz, est, 301)[0]
    cur = oracle.avg_current(le, 1)[0]
    up = oracle.upsampler(cur, 16, 4784)[0]
    av = oracle.moving_window_multi(up, 48, 3, 0)[0]
    tmin, tmax, amin, amax, _ = oracle.min_max(av)
    assert np.max(np.abs(out["A_max"] - amax) / np.abs(amax)) <= 1e-5
    assert np.all(np.abs(out["tp_aoe_samp"] - (est + tmax / 16)) <= 1.0)


def test_interpolated_threshold_times_in_a_recipe():
    """interpolated_time_point_thresh inside a chain: thresholds from numpy.amax of a trapezoid, start from min_max, the time written in
    ns with the linear interpolation between samples (the docstring example of the reference, time_point_thresh.py:152-167)"""
    from dspeed_amd.processing_chain import WaveformInput

    rng = np.random.default_rng(33)
    x, bl, t0 = _synth(rng, 64, 4096)
    wf = x.astype(np.float32)
    M = "dspeed.processors"
    rec = {"outputs": ["tp_50", "tp_50_i"], "processors": {
        "wf_blsub": f"{M}.bl_subtract(waveform, baseline, wf_blsub)",
        "wf_pz": f"{M}.pole_zero(wf_blsub, 27.46*us, wf_pz)",
        "wf_atrap": f"{M}.asym_trap_filter(wf_pz, 128*ns, 64*ns, 2*us, wf_atrap)",
        "t_lo, t_hi, a_lo, a_hi": {"function": "min_max", "module": M, "args": ["wf_atrap", "t_lo", "t_hi", "a_lo", "a_hi"],
                                   "unit": ["ns", "ns", "ADC", "ADC"]},
        "tp_50": {"function": "interpolated_time_point_thresh", "module": M, "unit": "ns",
                  "args": ["wf_atrap", "0.5*a_hi", "t_hi", 0, "'l'", "tp_50"]},
        "tp_50_i": {"function": "interpolated_time_point_thresh", "module": M, "unit": "ns",
                    "args": ["wf_atrap", "0.5*a_hi", "t_hi", 0, "'i'", "tp_50_i"]}}}
    _, out = _run(rec, {"waveform": WaveformInput(wf, 16.0, 1600.0), "baseline": bl})
    at = oracle.asym_trap_filter(oracle.pole_zero(oracle.bl_subtract(wf, bl)[0], np.float32(27460.0 / 16))[0], 8, 4, 125)[0]
    _, thi, _, ahi, _ = oracle.min_max(at)
    for mode, key in (("l", "tp_50"), ("i", "tp_50_i")):
        idx = oracle.interpolated_time_point_thresh(at, np.float32(0.5) * ahi, thi, 0, mode)[0]
        want = ((idx.astype(np.float64) + 100.0) * 16.0).astype(np.float32)
        same = out[key] == want
        assert same.mean() >= 0.9 and np.nanmax(np.abs(out[key] - want)) <= 32.0, key
    assert np.all(out["tp_50"] >= out["tp_50_i"]) and np.all(out["tp_50"] <= out["tp_50_i"] + 16.0)


def test_numpy_constants_and_ufuncs_in_recipes():
    """test_numpy_math_constants_dsp of the reference (tests/test_processing_chain.py:120-142) restated, in both spellings its
    configs use (inline expressions; numpy.subtract processors, tests/configs/numpy-parsing.json), on a float64 column"""
    n = 500
    ts = np.random.default_rng(2).uniform(1.5e9, 1.6e9, n)
    rec = {"outputs": ["timestamp", "calc1", "calc2", "calc3", "calc4", "calc5", "calc6", "d1", "d2", "d4"], "processors": {
        "calc1": "np.pi*timestamp", "calc2": "np.pi", "calc3": "np.pi*np.e", "calc4": "np.nan", "calc5": "np.inf", "calc6": "np.nan*timestamp",
        "d1": {"function": "subtract", "module": "numpy", "args": ["timestamp-timestamp", "np.pi*timestamp", "d1"]},
        "d2": {"function": "subtract", "module": "numpy", "args": ["timestamp-timestamp", "np.pi", "d2"]},
        "d4": {"function": "divide", "module": "numpy", "args": ["timestamp", "np.e*timestamp", "d4"]}}}
    chain, out = _run(rec, {"timestamp": ts})
    assert chain.loop_dtype == np.float64 and chain.program.slots == []
    assert np.array_equal(out["timestamp"], ts) and np.array_equal(out["calc1"], np.pi * ts)
    assert np.all(out["calc2"] == np.pi) and np.all(out["calc3"] == np.pi * np.e)
    assert np.isnan(out["calc4"]).all() and np.isinf(out["calc5"]).all() and np.isnan(out["calc6"]).all()
    assert np.array_equal(out["d1"], (ts - ts) - np.pi * ts) and np.array_equal(out["d2"], (ts - ts) - np.pi)
    assert np.array_equal(out["d4"], ts / (np.e * ts))


def test_tutorial_recipe_with_numpy_processors():
    """The shape of the reference's tutorial recipe (docs/source/notebooks/metadata/dsp-config.json): the baseline comes from
    linear_slope_fit and is removed with numpy.subtract -- a ufunc, so a NaN sample stays one sample instead of voiding the waveform
    as bl_subtract does --, energies with numpy.amax, A/E with numpy.divide."""
    from dspeed_amd.processing_chain import WaveformInput

    rng = np.random.default_rng(44)
    x, _bl, t0 = _synth(rng, 96, 4096)
    wf = x.astype(np.float32)
    M = "dspeed.processors"
    rec = {"outputs": ["trapEmax", "bl_mean", "A_10", "AoE", "wf_blsub", "wf_plus"], "processors": {
        "bl_mean , bl_sig, bl_slope, bl_intercept": {"function": "linear_slope_fit", "module": M, "unit": ["ADC"] * 4,
                                                      "args": ["waveform[0: 1000]", "bl_mean", "bl_sig", "bl_slope", "bl_intercept"]},
        "wf_blsub": {"function": "subtract", "module": "numpy", "args": ["waveform", "bl_mean", "wf_blsub"], "unit": "ADC"},
        "wf_plus": {"function": "add", "module": "numpy", "args": ["waveform", "bl_mean", "wf_plus"], "unit": "ADC"},
        "wf_pz": {"function": "pole_zero", "module": M, "args": ["wf_blsub", "db.pz_const", "wf_pz"], "defaults": {"db.pz_const": "27.46*us"}},
        "wf_trap": {"function": "trap_norm", "module": M, "args": ["wf_pz", "8*us", "4*us", "wf_trap"]},
        "trapEmax": {"function": "amax", "module": "numpy", "args": ["wf_trap", 1, "trapEmax"], "kwargs": {"signature": "(n),()->()", "types": ["fi->f"]}},
        "curr10": {"function": "avg_current", "module": M, "args": ["wf_pz", 10, "curr10(len(wf_pz)-10, 'f')"]},
        "A_10": {"function": "amax", "module": "numpy", "args": ["curr10", 1, "A_10"]},
        "AoE": {"function": "divide", "module": "numpy", "args": ["A_10", "trapEmax", "AoE"], "unit": "1/sample"}}}
    _, out = _run(rec, {"waveform": WaveformInput(wf, 16.0)})
    bm = oracle.linear_slope_fit(wf[:, :1000])[0]
    assert np.max(np.abs(out["bl_mean"] - bm) / np.abs(bm)) <= 1e-5
    blsub = wf - out["bl_mean"][:, None]
    assert np.array_equal(out["wf_blsub"], blsub) and np.array_equal(out["wf_plus"], wf + out["bl_mean"][:, None])
    pz = oracle.pole_zero(blsub, np.float32(27460.0 / 16))[0]
    emax = np.max(oracle.trap_norm(pz, 500, 250)[0], axis=1)
    a10 = np.max(oracle.avg_current(pz, 10)[0], axis=1)
    assert np.max(np.abs(out["trapEmax"] - emax) / emax) <= 1e-6 and np.max(np.abs(out["A_10"] - a10) / a10) <= 1e-5
    assert np.array_equal(out["AoE"], out["A_10"] / out["trapEmax"])
    # one NaN sample: numpy.subtract keeps it one sample (stored as such), everything downstream of it is NaN like the reference
    wf2 = wf.copy()
    wf2[3, 2000] = np.nan
    _, out2 = _run(rec, {"waveform": WaveformInput(wf2, 16.0)})
    want = wf2 - out2["bl_mean"][:, None]
    assert np.array_equal(np.isnan(out2["wf_blsub"]), np.isnan(want)) and np.isnan(out2["wf_blsub"][3]).sum() == 1
    assert np.array_equal(np.nan_to_num(out2["wf_blsub"]), np.nan_to_num(want))
    assert np.isnan(out2["trapEmax"][3]) and np.isnan(out2["AoE"][3]) and not np.isnan(np.delete(out2["AoE"], 3)).any()


def test_in_kernel_op_profile():
    """dsp_chain_profile: per-op shader-clock cycles from inside the one kernel a chain is; results are unchanged by it"""
    rng = np.random.default_rng(5)
    x, bl, t0 = _synth(rng, 2048, 4096)
    wf = x.astype(np.float32)
    tb = {"waveform": wf, "baseline": bl, "t_pick": (t0 + 700).astype(np.float32)}
    chain, out = _run(recipes.C2, tb)
    ref = out["trapEftp"].copy()
    c = chain._chain
    c.set_fused(0)  # the interpreter: the specialised kernels have no ops to time
    chain.execute()
    vm = out["trapEftp"].copy()
    c.profile(True)
    chain.execute()
    pr = c.profile_read()
    assert np.array_equal(out["trapEftp"], vm) and np.max(np.abs(vm - ref) / np.abs(ref)) <= TOL
    # (the BL_SUBTRACT right behind the LOAD is done by the load: dsp_chain_create takes it out of the device program)
    assert pr["opcodes"] == [o[0] for o in chain.program.ops if o[0] != _LIB.OP_BL_SUBTRACT] and len(pr["cycles"]) == len(pr["opcodes"])
    assert 0 < pr["waveforms"] <= 2048 and all(cy > 0 for cy in pr["cycles"])
    heavy = pr["opcodes"][int(np.argmax(pr["cycles"]))]
    assert heavy in (_LIB.OP_TRAP_PICKOFF, _LIB.OP_POLE_ZERO, _LIB.OP_LOAD)
    c.profile(False)
    with pytest.raises(Exception):
        c.profile_read()


def test_current_branch_recipe_pieces():
    """windower -> avg_current -> min_max (the first steps of the A/E branch, icpc-dsp-config.json:294-346) and trap_pickoff in one
    recipe; a window that reaches past the input makes NaN samples there, and every consumer of it NaN, as in the reference"""
    rng = np.random.default_rng(31)
    x, bl, t0 = _synth(rng, 90, 4096)
    wf = x.astype(np.float32)
    start = (t0 - 1000).astype(np.float32)
    start[3] = 4000.0  # window runs off the end
    M = "dspeed.processors"
    rec = {"outputs": ["wf_win", "a_max", "t_amax", "ct"], "processors": {
        "wf_pz": f"{M}.pole_zero(waveform, 1716.28, wf_pz)",
        "wf_win": f"{M}.windower(wf_pz, w_start, wf_win(2000, 'f'))",
        "curr": f"{M}.avg_current(wf_win, 5, curr(1995, 'f'))",
        "t_amin, t_amax, a_min, a_max": {"function": "min_max", "module": M, "args": ["curr", "t_amin", "t_amax", "a_min", "a_max"]},
        "ct": f"{M}.trap_pickoff(wf_pz, 94, 0, t_ct, ct)"}}
    tct = np.floor(t0 + 200).astype(np.float32)
    _, out = _run(rec, {"waveform": wf, "w_start": start, "t_ct": tct})
    pz = oracle.pole_zero(wf, 1716.28)[0]
    win = oracle.windower(pz, start, 2000)[0]
    assert np.array_equal(np.isnan(out["wf_win"]), np.isnan(win)) and np.isnan(win[3]).any() and not np.isnan(win[3]).all()
    assert_rel_to_peak(np.nan_to_num(out["wf_win"]), np.nan_to_num(win), TOL, "wf_win")
    cur = oracle.avg_current(np.nan_to_num(win), 5)[0]
    tmin, tmax, amin, amax, _ = oracle.min_max(cur)
    ok = np.ones(90, dtype=bool)
    ok[3] = False
    assert np.isnan(out["a_max"][3]) and np.isnan(out["t_amax"][3])
    assert np.max(np.abs(out["a_max"][ok] - amax[ok]) / np.abs(amax[ok])) <= 1e-5
    ct = oracle.trap_pickoff(pz, 94, 0, tct)[0]
    assert np.max(np.abs(out["ct"] - ct) / np.max(np.abs(pz), axis=1)) <= TOL


def test_host_buffers_stream_through_in_overlapped_pieces():
    """Host-resident columns are processed in pieces (H2D of piece k+1 overlaps kernel and D2H of piece k): same results as one
    piece, a waveform-valued output included, an output column of another dtype converted, a data-dependent DSPFatal reported
    with its absolute row."""
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processing_chain import build_processing_chain

    rng = np.random.default_rng(15)
    n = 1000
    x, bl, t0 = _synth(rng, n, 4096)
    wf = x.astype(np.float32)
    tp = (t0 + 625 + 150.4).astype(np.float32)
    want, _ = oracle.chain_energy(wf, bl, tp, 1716.28, 625, 188, "l")
    tb = {"waveform": wf, "baseline": bl, "t_pick": tp}
    chain, _, tb_out = build_processing_chain(recipes.C2, tb)
    chain.execute()
    one_piece = tb_out["trapEftp"].copy()
    assert np.max(np.abs(one_piece - want) / np.abs(want)) <= TOL
    chain.pipeline_bytes = 37 * 4096 * 4  # 37-row pieces: 28 pieces, the last one ragged
    tb_out["trapEftp"][:] = 0
    chain.execute()
    assert np.array_equal(tb_out["trapEftp"], one_piece)
    out64 = {"trapEftp": np.zeros(n, dtype=np.float64)}  # a column of another dtype is filled through a converted copy
    chain(tb, out64)
    assert np.array_equal(out64["trapEftp"], one_piece.astype(np.float64))
    # waveform-valued output + error row attribution across pieces
    c1, _, o1 = build_processing_chain(recipes.C1, {"waveform": wf[:, :1024].copy()})
    c1.execute()
    ref = o1["wf_trap"].copy()
    c1.pipeline_bytes = 64 * 1024 * 4 * 2
    o1["wf_trap"][:] = 0
    c1.execute()
    assert np.array_equal(o1["wf_trap"], ref)
    tpi = np.floor(tp).astype(np.float32)
    tpi[777] += 0.5
    ci, _, _ = build_processing_chain({"outputs": ["e"], "processors": {
        "wf_t": "dspeed.processors.trap_filter(waveform, 100, 10, wf_t)",
        "e": "dspeed.processors.fixed_time_pickoff(wf_t, t_pick, 'i', e)"}}, {"waveform": wf, "t_pick": tpi})
    ci.pipeline_bytes = 100 * 4096 * 4
    with pytest.raises(DSPFatal) as ei:
        ci.execute()
    assert ei.value.wf_range == range(777, 778)


_PICKOFF_AT_INTEGERS = {"outputs": ["e"], "processors": {
    "wf_t": "dspeed.processors.trap_filter(waveform, 100, 10, wf_t)",
    "e": "dspeed.processors.fixed_time_pickoff(wf_t, t_pick, 'i', e)"}}


def _rows_with_integer_pickoffs(n=1000):
    x, _bl, t0 = _synth(np.random.default_rng(15), n, 4096)
    return x.astype(np.float32), np.floor(t0 + 625 + 150.4).astype(np.float32)


def test_a_chain_runs_again_after_a_failed_pass_over_pieces():
    """what the cleanup of a failed pass leaves behind: with the bad row mended in the linked column the same chain runs, raises nothing and
    gives a fresh chain's output bit for bit (no error word, transfer or kernel of the abandoned pieces meets the next pass)"""
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processing_chain import build_processing_chain

    wf, tpi = _rows_with_integer_pickoffs()
    good = tpi[777]
    tpi[777] += 0.5
    tb = {"waveform": wf, "t_pick": tpi}
    ci, _, out = build_processing_chain(_PICKOFF_AT_INTEGERS, tb)
    ci.pipeline_bytes = 100 * 4096 * 4
    with pytest.raises(DSPFatal) as ei:
        ci.execute()
    assert ei.value.wf_range == range(777, 778)
    tpi[777] = good
    out["e"][:] = 0
    ci.execute()
    fresh, _, want = build_processing_chain(_PICKOFF_AT_INTEGERS, tb)
    fresh.execute()
    assert np.array_equal(out["e"], want["e"], equal_nan=True) and np.isfinite(want["e"]).all()


def test_the_first_bad_row_in_table_order_is_the_one_reported():
    """two bad rows in different pieces: the pieces are finished in order, so the DSPFatal names the earlier row"""
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processing_chain import build_processing_chain

    wf, tpi = _rows_with_integer_pickoffs()
    tpi[777] += 0.5
    tpi[123] += 0.5
    ci, _, _ = build_processing_chain(_PICKOFF_AT_INTEGERS, {"waveform": wf, "t_pick": tpi})
    ci.pipeline_bytes = 100 * 4096 * 4
    with pytest.raises(DSPFatal) as ei:
        ci.execute()
    assert ei.value.wf_range == range(123, 124)


def test_fatal_from_recipe_carries_processor_context():
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processing_chain import build_processing_chain

    bad = {"outputs": ["wf_t"], "processors": {"wf_t": "dspeed.processors.trap_filter(waveform, 3000, 10, wf_t)"}}
    chain, _, _ = build_processing_chain(bad, {"waveform": np.zeros((4, 4096), dtype=np.float32)})
    with pytest.raises(DSPFatal, match="wider than the waveform"):
        chain.execute()


def test_float64_inputs_run_the_float64_chain():
    """A float64 waveform column selects the float64 loops for the whole recipe; outputs come back as float64."""
    rng = np.random.default_rng(8)
    x, bl, t0 = _synth(rng, 40, 4096)
    tp = (t0 + 625 + 150.4)
    chain, out = _run(recipes.C2_UNITS, {"waveform": __import__("dspeed_amd.processing_chain", fromlist=["WaveformInput"]).WaveformInput(x, dt=16.0),
                                         "baseline": bl.astype(np.float64), "t_pick": tp})
    assert out["trapEftp"].dtype == np.float64 and out["wf_trap"].dtype == np.float64
    xb = oracle.bl_subtract(x, bl.astype(np.float64))[0]
    tr = oracle.trap_filter(oracle.pole_zero(xb, 27460.5 / 16.0)[0], 625, 188)[0]
    assert_rel_to_peak(out["wf_trap"], tr, 1e-12, "wf_trap f64")
    e = oracle.fixed_time_pickoff(tr, tp, "l")[0]
    assert np.max(np.abs(out["trapEftp"] - e) / np.abs(e)) <= 1e-12


@pytest.mark.parametrize("L,num,typ", [(48, 3, 0), (48, 1, 2), (7, 2, 1), (1, 4, 0), (80, 3, 0), (75, 2, 2), (300, 2, 0)])
@pytest.mark.parametrize("n", [4784, 4096, 1000])
def test_moving_window_multi_in_a_chain_in_place_and_between_two_buffers(L, num, typ, n):
    """a source nobody reads again is overwritten pass by pass when the window fits a lane's chunk (DSP_OP_MOVING_WINDOW_MULTI ip[3] = 1),
    else the passes go between two buffers; both against the oracle, and a neighbouring waveform of the same program stays intact"""
    from dspeed_amd import _lib
    from dspeed_amd.processing_chain import build_processing_chain

    rng = np.random.default_rng(L * 100 + num * 10 + typ + n)
    x = (50 * rng.standard_normal((200, n)) + 2000 * np.exp(-((np.arange(n)[None, :] - rng.uniform(0.3 * n, 0.7 * n, (200, 1))) / 200.0) ** 2)).astype(np.float32)
    x[5, 7] = np.nan
    bl = rng.uniform(-50, 50, 200).astype(np.float32)
    M = "dspeed.processors"
    rec = {"outputs": ["wf_mw", "t_lo", "t_hi", "a_lo", "a_hi"], "processors": {
        "t_lo, t_hi, a_lo, a_hi": f"{M}.min_max(waveform, t_lo, t_hi, a_lo, a_hi)",  # (registers written before the averages run)
        "wf_bl": f"{M}.bl_subtract(waveform, baseline, wf_bl)",
        "wf_mw": f"{M}.moving_window_multi(wf_bl, {L}, {num}, {typ}, wf_mw)"}}
    chain, _, out = build_processing_chain(rec, {"waveform": x, "baseline": bl})
    mw = [o for o in chain.program.ops if o[0] == _lib.OP_MOVING_WINDOW_MULTI][0]
    chunk = -(-(-(-n // 64)) // 16) * 16
    in_place = len(mw[4]) > 3 and mw[4][3] == 1
    assert in_place == (L <= chunk) and (mw[1] == mw[2]) == in_place
    chain.execute()
    xb = oracle.bl_subtract(x, bl)[0]
    want = oracle.moving_window_multi(xb, L, num, typ)[0]
    ok = ~np.isnan(want).all(axis=1)
    peak = np.nanmax(np.abs(np.where(ok[:, None], want, 0.0)), axis=1, keepdims=True)
    assert np.array_equal(np.isnan(out["wf_mw"]), np.isnan(want))
    assert np.nanmax(np.abs(out["wf_mw"][ok] - want[ok]) / peak[ok]) <= 1e-6
    tl, th, al, ah = oracle.min_max(x)[:4]
    for k, w in (("t_lo", tl), ("t_hi", th), ("a_lo", al), ("a_hi", ah)):
        assert np.array_equal(out[k], w, equal_nan=True), k
