"""The planner's and the recipe compiler's part of histogram / histogram_stats without a device (dsp_chain_plan): DSP_OP_HISTOGRAM and
DSP_OP_HISTOGRAM_STATS have one route -- dsp_hist_kernel, whatever the switches say --, exactly three program shapes, and every refusal by
name; the registry, the C ABI and the module strings of the reference's recipes; the stage list of the SiPM fragment."""
import ctypes

import numpy as np
import pytest

import histogram_cases as hc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import DSPFatal

M = "dspeed.processors"


def test_the_three_shapes_take_the_histogram_kernel_whatever_the_switches_say(monkeypatch):
    shapes = [(hc.hist_program(1000, 100), np.float32), (hc.hist_program(1000, 100, stats=True), np.float32),
              (hc.hist_program(1024, hc.MAX_BINS, np.int16, stats=True, stores=False, max_in="column"), np.float32),
              (hc.hist_program(1000, 65, np.uint16, offset=3, row_stride=1007), np.float32), (hc.stats_program(100), np.float32),
              (hc.stats_program(1, max_in="column"), np.float32), (hc.hist_program(257, 64, np.float64, np.float64, stats=True), np.float64),
              (hc.stats_program(65, np.float64, max_in=0.5), np.float64)]
    for p, loop in shapes:
        assert plan(p, loop)["kernel"] == "dsp_hist_kernel"
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    assert plan(shapes[0][0])["kernel"] == "dsp_hist_kernel"
    # the kernel keeps no row in LDS: rows of 2^20 samples (the longest a slot describes; weights count them exactly in float32), float64 rows of 100 000
    assert plan(hc.hist_program(1 << 20, 100))["kernel"] == "dsp_hist_kernel"
    assert plan(hc.hist_program(100000, 100, np.float64, np.float64), np.float64)["kernel"] == "dsp_hist_kernel"


def test_any_other_program_with_either_op_is_refused_by_name():
    shape = "DSP_OP_HISTOGRAM / DSP_OP_HISTOGRAM_STATS.*histogram, histogram_stats.*dsp_hist_kernel only.*LOAD, HISTOGRAM, STORE, STORE"
    p = hc.hist_program(1000, 100)
    p.ops.pop()  # one store only
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = hc.hist_program(1000, 100)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = hc.hist_program(1000, 100, stats=True)
    p.ops.pop()  # two of the three per-event values
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = hc.hist_program(1000, 100, stats=True)
    p.n_sregs = 4
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=0)
    with pytest.raises(NotImplementedError, match="DSP_OP_HISTOGRAM"):
        plan(p)
    p = hc.hist_program(1000, 100, stats=True)  # histogram_stats of something else than the histogram beside it
    p.slots += [100, 101]
    op = list(p.ops[2])
    op[2], op[4] = 3, (4, 0)
    p.ops[2] = tuple(op)
    with pytest.raises(NotImplementedError, match="DSP_OP_HISTOGRAM"):
        plan(p)
    with pytest.raises(NotImplementedError, match="the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
        plan(hc.hist_program(1000, 100, np.int32, np.float64), np.float64)
    p = hc.stats_program(100)
    p.ops[3] = p.ops[3][:4] + ((2,),) + p.ops[3][5:]  # fwhm stored twice, mode never
    with pytest.raises(NotImplementedError, match="mode_out, max_out and fwhm_out are stored once each"):
        plan(p)
    p = hc.hist_program(1000, 100, stats=True)
    op = list(p.ops[2])
    op[5] = (Scalar.reg(0),)
    p.ops[2] = tuple(op)
    with pytest.raises(NotImplementedError, match="max_in is a constant or a per-event column of the loop's type"):
        plan(p)


def test_the_reference_s_checks_and_the_bounds():
    for borders_len in (100, 102):
        with pytest.raises(DSPFatal, match="length borders_out must be exactly 1 \\+ length of weights_out"):
            plan(hc.hist_program(1000, 100, borders_len=borders_len))
    with pytest.raises(DSPFatal, match="length edges_in must be exactly 1 \\+ length of weights_in"):
        plan(hc.stats_program(100, edges_len=100))
    plan(hc.hist_program(1000, hc.MAX_BINS))
    with pytest.raises(NotImplementedError, match=f"histogram: at most {hc.MAX_BINS} bins \\({hc.MAX_BINS + 1} asked for\\)"):
        plan(hc.hist_program(1000, hc.MAX_BINS + 1))
    with pytest.raises(NotImplementedError, match=f"histogram_stats: at most {hc.MAX_BINS} bins"):
        plan(hc.stats_program(hc.MAX_BINS + 1))
    with pytest.raises(ValueError, match="at most 2\\^20 samples"):  # (every slot's bound, well inside the 2^24 a float32 weight counts exactly)
        plan(hc.hist_program((1 << 20) + 1, 100))


def test_registry_abi_and_messages():
    from dspeed_amd import processors

    assert "histogram" in processors.__all__ and "histogram_stats" in processors.__all__
    g = processors.histogram
    assert g.signature == "(n),(m),(p)" and g.types == ["fff", "ddd"] and (g.nin, g.nout) == (3, 0)
    g = processors.histogram_stats
    assert g.signature == "(n),(m),(),(),(),()" and g.types == ["ffffff", "dddddd"] and (g.nin, g.nout) == (6, 0)
    with pytest.raises(TypeError, match="both outputs must be passed"):
        processors.histogram(np.zeros(10, np.float32))
    with pytest.raises(TypeError, match="the three outputs stand in the middle"):
        processors.histogram_stats(np.zeros(4, np.float32), np.zeros(5, np.float32), np.nan)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, f"dsp_{name}_{sfx}") for name in ("histogram", "histogram_stats") for sfx in ("f32", "f64"))
    assert (_lib.OP_HISTOGRAM, _lib.OP_HISTOGRAM_STATS) == (35, 36)
    L.dsp_fatal_message.restype = ctypes.c_char_p
    assert [L.dsp_fatal_message(c).decode() for c in (29, 30)] == ["length borders_out must be exactly 1 + length of weights_out",
                                                                 "length edges_in must be exactly 1 + length of weights_in"]


def test_module_strings_name_the_package_or_the_file_that_defines_the_processor():
    from dspeed_amd import processors
    from dspeed_amd.language import _PROCESSOR_FILES, module_accepted

    assert sorted(_PROCESSOR_FILES) == sorted(processors.__all__)  # a file for every processor the registry has
    for fn, files in _PROCESSOR_FILES.items():
        assert module_accepted("dspeed.processors", fn) and module_accepted("dspeed_amd.processors", fn)
        assert all(module_accepted(f"dspeed.processors.{f}", fn) for f in files)
    assert module_accepted("dspeed.processors.histogram", "histogram_stats") and module_accepted("dspeed.processors.histogram_stats", "histogram_stats")
    assert module_accepted("dspeed.processors.moving_windows", "avg_current") and module_accepted("dspeed.processors.trap_filters", "trap_norm")
    assert not module_accepted("dspeed.processors.histogram_stats", "histogram") and not module_accepted("dspeed.processors.nothing", "histogram")
    assert not module_accepted("dspeed.processors.histogram.deeper", "histogram") and not module_accepted("scipy.signal", "histogram")
    from dspeed_amd.processing_chain import build_processing_chain

    tb = {"waveform": np.zeros((4, 64), np.float32)}
    with pytest.raises(NotImplementedError, match="module 'dspeed.processors.bl_subtract' is not available on the device path \\(processor dspeed.processors.bl_subtract.min_max\\)"):
        build_processing_chain({"outputs": ["a"], "processors": {"t, u, a, b": {"function": "min_max", "module": "dspeed.processors.bl_subtract",
                                                                               "args": ["waveform", "t", "u", "a", "b"]}}}, tb)


def test_the_sipm_fragment_is_one_fused_launch_ahead_of_the_peak_finder(monkeypatch):
    from dspeed_amd.processing_chain import build_processing_chain

    tb = {"waveform": np.random.default_rng(5).integers(0, 1000, (12, 1000)).astype(np.uint16)}
    chain, _, out = build_processing_chain({"outputs": ["vt_max_candidate_out", "n_max_out", "fwhm"], "processors": hc.sipm_fragment()}, tb)
    stages = [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]
    kernels = [k for _, k, _ in stages]
    assert kernels.count("dsp_hist_kernel") == 1 and kernels.count("dsp_extrema_kernel") == 1
    assert kernels.index("dsp_hist_kernel") < kernels.index("dsp_scalar_kernel") < kernels.index("dsp_extrema_kernel")  # 3*fwhm in between
    what, _, ops = stages[kernels.index("dsp_hist_kernel")]
    assert "histogram" in what and "histogram_stats" in what and "one launch" in what
    # no weight or border leaves the launch when the recipe does not ask for them
    assert ops == [_lib.OP_LOAD, _lib.OP_HISTOGRAM, _lib.OP_HISTOGRAM_STATS] + [_lib.OP_STORE_SCALAR] * 3
    assert stages[0][0].startswith("curr -> HBM") and out["fwhm"].dtype == np.float32 and out["vt_max_candidate_out"].shape == (12, 20)
    # ... and both when it does
    chain, _, out = build_processing_chain({"outputs": ["fwhm", "hist_weights", "idx_out_c"], "processors": hc.sipm_fragment()}, tb)
    ops = next([op[0] for op in st["program"].ops] for st in chain._stages if plan(st["program"])["kernel"] == "dsp_hist_kernel")
    assert ops == [_lib.OP_LOAD, _lib.OP_HISTOGRAM, _lib.OP_HISTOGRAM_STATS, _lib.OP_STORE, _lib.OP_STORE] + [_lib.OP_STORE_SCALAR] * 3
    assert out["hist_weights"].shape == (12, 100)
    # histogram alone, and histogram_stats of rows that are chain inputs
    procs = {k: v for k, v in hc.sipm_fragment("waveform").items() if k.startswith(("curr", "hist_"))}
    chain, _, out = build_processing_chain({"outputs": ["hist_weights", "hist_borders"], "processors": procs}, tb)
    ops = next([op[0] for op in st["program"].ops] for st in chain._stages if plan(st["program"])["kernel"] == "dsp_hist_kernel")
    assert ops == [_lib.OP_LOAD, _lib.OP_HISTOGRAM, _lib.OP_STORE, _lib.OP_STORE] and out["hist_borders"].shape == (12, 101)
    tb2 = {"w": np.ones((12, 100), np.float32), "e": np.ones((12, 101), np.float32)}
    chain, _, out = build_processing_chain({"outputs": ["fwhm"], "processors": {"fwhm, idx, mx": {
        "function": "histogram_stats", "module": f"{M}.histogram_stats", "args": ["w", "e", "idx", "mx", "fwhm", 0.5]}}}, tb2)
    ops = next([op[0] for op in st["program"].ops] for st in chain._stages if plan(st["program"])["kernel"] == "dsp_hist_kernel")
    assert ops == [_lib.OP_LOAD, _lib.OP_LOAD, _lib.OP_HISTOGRAM_STATS] + [_lib.OP_STORE_SCALAR] * 3
    # refusals, by name
    bad = hc.sipm_fragment()
    bad["hist_weights , hist_borders"]["args"] = ["curr", "hist_weights(100)", "hist_borders(100)"]
    with pytest.raises(DSPFatal, match="length borders_out must be exactly 1 \\+ length of weights_out"):
        build_processing_chain({"outputs": ["fwhm"], "processors": bad}, tb)
    bad = hc.sipm_fragment()
    bad["hist_weights , hist_borders"]["args"] = ["curr", "hist_weights(4000)", "hist_borders(4001)"]
    with pytest.raises(NotImplementedError, match="histogram.*at most 2048 bins"):
        build_processing_chain({"outputs": ["fwhm"], "processors": bad}, tb)
    for fn in ("histogram_around_mode", "histogram_peakstats", "gaussian_filter1d", "peak_snr_threshold", "multi_a_filter"):
        with pytest.raises(NotImplementedError, match=f"processor '{fn}' is not implemented on the device path"):
            build_processing_chain({"outputs": ["x"], "processors": {"x": {"function": fn, "module": M, "args": ["waveform", "x"]}}}, tb)
    with pytest.raises(NotImplementedError, match="histogram in a recipe whose loop type is float64"):
        build_processing_chain({"outputs": ["hist_weights"], "processors": procs}, {"waveform": tb["waveform"].astype(np.float64)})
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="histogram.*DSPEED_HIP_NO_STAGES"):
        build_processing_chain({"outputs": ["fwhm"], "processors": hc.sipm_fragment()}, tb)
