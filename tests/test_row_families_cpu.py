"""The waveform families of tests/row_families.py on the CPU: the generator is deterministic, every family has the property that defines it,
and on every route of tests/test_gpu_row_families.py the oracle ALONE returns code 0 on every row and leaves each output finite in at least
half of a batch's rows and in every `control` row -- so that the device comparison is never NaN against NaN for most of a batch."""
import functools

import numpy as np
import pytest

import oracle
import recipes
import row_families as rf
import row_family_routes as routes

DTYPES = [np.int16, np.uint16, np.float32]
ids = lambda v: getattr(v, "__name__", str(v))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _batch(n, dtype, layout="interleaved", collect=0.0):
    return rf.interleaved(n, dtype, collect=collect) if layout == "interleaved" else rf.sorted_runs(n, dtype, collect=collect)


def test_generator_is_deterministic_and_laid_out_as_promised():
    for dtype in DTYPES:
        a, b = rf.interleaved(2048, dtype), rf.interleaved(2048, dtype)
        assert a.rows.dtype == dtype and np.array_equal(a.rows, b.rows) and np.array_equal(a.family, b.family)
        assert np.array_equal(a.pedestal, b.pedestal) and np.array_equal(a.onset, b.onset, equal_nan=True)
        assert not np.array_equal(a.rows, rf.interleaved(2048, dtype, seed=1).rows)
        assert len(a) == 131 and len(a) % 64 != 0 and set(a.family) == set(rf.FAMILIES)
        for lo in range(0, 128, 64):  # every wavefront of a lane-per-row kernel holds mixed families
            assert len(set(a.family[lo:lo + 64])) >= 10
        s = rf.sorted_runs(2048, dtype)
        assert len(s) == 64 * len(rf.FAMILIES)
        for k, name in enumerate(rf.FAMILIES):  # whole wavefronts of one family
            assert (s.family[64 * k:64 * (k + 1)] == name).all()
        # a family's rows do not depend on what else is in the batch
        assert np.array_equal(s.rows[s.of("pileup")][:8], rf.family("pileup", 2048, dtype, 64).rows[:8])


@pytest.mark.parametrize("n", [2048, 8192])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_every_family_has_its_defining_property(dtype, n):
    rows = 12
    lo, hi = rf.sample_range(dtype)
    fam = {name: rf.family(name, n, dtype, rows) for name in rf.FAMILIES}
    x = {name: b.rows.astype(np.float64) - b.pedestal[:, None].astype(np.float64) for name, b in fam.items()}  # above the pedestal
    at = lambda name, offset: x[name][np.arange(rows), (fam[name].onset + offset).astype(int)]  # noqa: E731
    for name, b in fam.items():
        assert b.rows.shape == (rows, n) and b.rows.dtype == dtype and b.rows.min() >= lo and b.rows.max() <= hi
        if np.dtype(dtype).kind in "iu" or name == "full_scale":
            assert np.array_equal(b.rows, np.rint(b.rows))
    mid = lambda b: ((0.45 * n - 1 <= b.onset) & (b.onset <= 0.55 * n)).all()  # noqa: E731
    # control: the suite's pulse -- a step of 500 .. 15000 mid-row over sigma-5 noise, decaying with TAU
    assert mid(fam["control"]) and (at("control", 0) > 450).all() and (at("control", 0) < 15050).all() and (np.abs(at("control", -1)) < 40).all()
    assert np.allclose(x["control"][:, :700].std(axis=1), rf.SIGMA, rtol=0.15)
    assert np.allclose(at("control", 800) / at("control", 0), np.exp(-800 / rf.TAU), atol=0.05)
    # noise_only / constant: no pulse
    assert np.isnan(fam["noise_only"].onset).all() and np.allclose(x["noise_only"].std(axis=1), rf.SIGMA, rtol=0.1)
    assert (np.abs(x["noise_only"]).max(axis=1) < 8 * rf.SIGMA).all()
    assert np.isnan(fam["constant"].onset).all() and (x["constant"] == 0).all()
    # noise_free: flat to the last bit ahead of the pulse
    assert mid(fam["noise_free"]) and (fam["noise_free"].rows[:, :700] == fam["noise_free"].rows[:, :1]).all() and (at("noise_free", 0) > 450).all()
    # saturated: a plateau of at least 100 samples at the top of the range, beginning mid-row
    sat = fam["saturated"].rows == dtype(hi)
    assert (sat.sum(axis=1) >= 100).all() and (np.argmax(sat, axis=1) == fam["saturated"].onset).all() and not sat[:, :700].any()
    # full_scale: integers, 80 .. 98 % of the headroom, nothing clipped, and float32 trapezoid sums beyond 2^24
    fs = fam["full_scale"]
    head = hi - fs.pedestal.astype(np.float64)
    assert (fs.rows < hi).all() and (fs.rows > lo).all() and (x["full_scale"].max(axis=1) > 0.79 * head).all() and (x["full_scale"].max(axis=1) < 0.99 * head).all()
    assert np.array_equal(fs.pedestal, np.rint(fs.pedestal))
    trap, rc = oracle.trap_filter(rf.family("full_scale", 8192, dtype, rows).rows.astype(np.float32), 1250, 376)
    assert rc == 0 and (np.abs(trap).max(axis=1) > 2 ** 24).all()
    trap, rc = oracle.trap_filter(rf.family("full_scale", 4096, dtype, rows).rows.astype(np.float32), 625, 188)
    assert rc == 0 and (np.abs(trap).max(axis=1) > 2 ** 24).all()
    # negative: the pulse goes down, nothing goes up, nothing is clipped
    assert (at("negative", 0) < -450).all() and (x["negative"].max(axis=1) < 8 * rf.SIGMA).all() and (fam["negative"].rows > lo).all()
    # pileup: two steps, 40 .. 1500 samples apart, both inside the row
    steps = np.diff(x["pileup"], axis=1) > 250
    assert (steps.sum(axis=1) == 2).all()
    gap = n - 1 - np.argmax(steps[:, ::-1], axis=1) - np.argmax(steps, axis=1)
    assert (gap >= 40).all() and (gap <= 1500).all() and (np.argmax(steps, axis=1) + 1 == fam["pileup"].onset).all()
    # tail: the row begins above its pedestal and falls, then the pulse
    assert (x["tail"][:, :50].mean(axis=1) > 60).all() and (x["tail"][:, :50].mean(axis=1) > x["tail"][:, 600:650].mean(axis=1)).all() and mid(fam["tail"])
    assert (at("tail", 0) - at("tail", -1) > 450).all()
    # early / late: the onset in the first eight samples / in the last 150
    assert (fam["early"].onset >= 0).all() and (fam["early"].onset <= 7).all() and (at("early", 0) > 450).all()
    assert (fam["late"].onset >= n - 150).all() and (fam["late"].onset <= n - 2).all() and (at("late", 0) > 450).all() and (np.abs(at("late", -1)) < 40).all()
    # tau_short / tau_long: half / twice the recipes' decay constant
    assert np.allclose(at("tau_short", 800) / at("tau_short", 0), np.exp(-800 / (0.5 * rf.TAU)), atol=0.05)
    assert np.allclose(at("tau_long", 800) / at("tau_long", 0), np.exp(-800 / (2.0 * rf.TAU)), atol=0.05)
    # slow_rise: half way up after 30 samples, at the top after 60
    assert np.allclose(at("slow_rise", 30) / at("slow_rise", 60), 0.5, atol=0.06) and (np.abs(at("slow_rise", 0)) < 40).all()
    # tiny: a step of 5 .. 30, comparable to the noise
    assert (x["tiny"][:, n // 2 + n // 16:].max(axis=1) < 60).all() and (x["tiny"].max(axis=1) < 75).all()
    step = np.array([x["tiny"][r, int(t):int(t) + 200].mean() - x["tiny"][r, int(t) - 200:int(t)].mean() for r, t in enumerate(fam["tiny"].onset)])
    assert (step > 2).all() and (step < 32).all()


# ---- the routes on the oracle alone: every call returns 0 (asserted where it is made, routes._ok), and the caps
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("n,rise,flat", [(4096, 625, 188), (1024, 64, 16)])
def test_r1_energy_chain_oracle(dtype, n, rise, flat):
    b = _batch(n, dtype)
    for mode in "lnh":
        _inp, want = routes.r1(b, rise, flat, mode)
        routes.check_caps(b, want, f"R1 {mode}")
        assert np.isnan(want["trapEftp"][b.of("late")]).any()  # (pick-off times beyond the row are in the batch)
        assert (want["_peak"][b.of("constant")] == 0).all()
    if n == 4096 and dtype == np.float32:  # (the batch of the GPU test's case with a time constant per event)
        _inp, want = routes.r1(b, rise, flat, "l", tau="per_event")
        routes.check_caps(b, want, "R1 per-event tau")


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=ids)
@pytest.mark.parametrize("n,layout,form,trap", routes.R2_FORMS, ids=ids)
def test_r2_rows_kernel_oracle(dtype, n, layout, form, trap):
    b = _batch(n, dtype, layout)
    inp, want = routes.r2(b, routes.DPZ if form == "C5" else routes.PZ, trap, form == "bl")
    routes.check_caps(b, want, "R2")
    thr, n_rows = inp["thr"], len(b)
    assert (thr < 0).any() and np.isfinite(thr).all()
    pulses = np.isin(b.family, rf.PULSE_FAMILIES) & ~b.of("negative") & ~b.of("noise_free")  # (an upward pulse over noise)
    assert np.isfinite(want["tp_0"][pulses]).mean() > 0.9, "the walks of the pulse families find crossings"
    assert n_rows == (131 if layout == "interleaved" else 64 * len(rf.FAMILIES))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_r3_extremes_and_walks_oracle(dtype):
    b = _batch(2048, dtype)
    _inp, want = routes.r3_pz(b)
    routes.check_caps(b, want, "R3 pz rows")
    inp, want = routes.r3_reduce(b)
    routes.check_caps(b, want, "R3 raw rows")
    sat = b.of("saturated")
    # a plateau's first sample wins, and the walk whose threshold is the plateau's value starts on it
    assert np.array_equal(want["t_max"][sat], b.onset[sat].astype(np.float32)) and (inp["thr"][sat] == want["a_max"][sat]).all()
    assert np.isfinite(want["walk0"][sat]).all()
    assert (want["t_max"][b.of("constant")] == 0).all() and (want["t_min"][b.of("constant")] == 0).all()


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=ids)
def test_r4_fir_oracle(dtype):
    b = _batch(8192, dtype)
    _inp, want = routes.r4_c3(b)
    routes.check_caps(b, want, "R4 C3")
    # where the pulse lies outside [:6092] or there is none, sum|k| max|x| is hundreds of times the filtered row's peak (the issue's 330 - 434
    # against 5 - 15): the dot-product term of the FIR bar is the one that binds there
    for nm in ("cusp", "zac"):
        ratio = want[f"_dot:{nm}"] / np.where(want[f"_peak:{nm}"] == 0, np.inf, want[f"_peak:{nm}"])
        assert (ratio[b.of("noise_only") | b.of("late")] > 60).all() and (ratio[b.of("control")] < 40).all(), nm
    if dtype == np.float32:
        inp, want = routes.r4_runs(b)
        routes.check_caps(b, want, "R4 t0 filter")
        assert np.isfinite(inp["thr"]).all()


@pytest.mark.parametrize("dtype", [np.uint16, np.int16], ids=ids)
@pytest.mark.parametrize("n,rise,flat", [(8192, 1250, 376), (4096, 625, 188)])
def test_r5_trapezoids_on_integer_rows_oracle(dtype, n, rise, flat):
    b = _batch(n, dtype)
    for case in routes.r5_cases(rise, flat):
        inp, want = routes.r5(b, case, rise, flat)
        routes.check_caps(b, want, f"R5 {case[0]}")
        f = want["wf_t"]
        if case[0] == "trap_filter":
            assert (np.abs(f[b.of("full_scale")]).max(axis=1) > 2 ** 24).all()


@pytest.mark.parametrize("layout", ["interleaved", "sorted"])
def test_r6_current_and_fits_oracle(layout):
    b = _batch(2048, np.float32, layout, 6.0)  # (the GPU test's batch)
    inp, want = routes.r6_current(b)
    routes.check_caps(b, want, "R6 current")
    assert np.isnan(want["a_hi"][b.of("early") | b.of("late")]).all()  # (window starts outside the row are in the batch)
    _inp, want = routes.r6_fits(b)
    routes.check_caps(b, want, "R6 fits")


@pytest.mark.parametrize("par", [recipes.ICPC_PARAMS, recipes.ICPC_REF_PARAMS], ids=["ICPC", "ICPC_REF"])
def test_r7_whole_recipe_oracle(par):
    from test_gpu_icpc_recipe import _expected  # (the all-oracle run of the recipe; NumPy and the oracle only)

    b = _batch(8192, np.uint16, collect=6.0)  # (a rise of some samples, as the whole-recipe tests draw it: a step has no rise-time ladder)
    want, _tp0 = _expected(b.rows, b.pedestal, routes.r7_t0_ns(len(b)), par=par)
    routes.check_caps(b, {k: v for k, v in want.items() if not k.startswith("_")}, "R7")
