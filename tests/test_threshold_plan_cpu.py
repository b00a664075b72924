"""The planner's and the recipe compiler's part of multi_time_point_thresh / time_over_threshold without a device (dsp_chain_plan):
DSP_OP_MULTI_TIME_POINT_THRESH and DSP_OP_TIME_OVER_THRESHOLD have one route -- dsp_thresh_kernel, whatever the switches say --, three
program shapes, and every refusal by name; the registry, the C ABI and the reference's module strings; the host's checks with the
reference's texts; the stage list of a rise-time recipe."""
import ctypes

import numpy as np
import pytest

import threshold_cases as tc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import DSPFatal

M = "dspeed.processors"
KERNEL = "dsp_thresh_kernel"


def test_the_shapes_take_the_threshold_kernel_whatever_the_switches_say(monkeypatch):
    shapes = [(tc.multi_program(1000, 3), np.float32), (tc.multi_program(1000, 64, np.int16, lists=True, t_start="column", polarity=-2.0, mode="r"), np.float32),
              (tc.multi_program(1000, 7, np.uint16, offset=3, row_stride=1007, mode="n"), np.float32), (tc.multi_program(2, 1, mode="i"), np.float32),
              (tc.multi_program(129, 20, np.float64, np.float64, lists=True, polarity=-1.0), np.float64),
              (tc.over_program(1000), np.float32), (tc.over_program(8192, np.uint16, threshold="column"), np.float32),
              (tc.over_program(65, np.float64, np.float64, threshold=np.nan), np.float64)]
    for p, loop in shapes:
        assert plan(p, loop)["kernel"] == KERNEL
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    assert plan(shapes[0][0])["kernel"] == KERNEL and plan(shapes[5][0])["kernel"] == KERNEL
    # the kernel keeps no row in LDS: rows of 2^20 samples (the longest a slot describes), float64 rows of 100 000
    assert plan(tc.multi_program(1 << 20, 3))["kernel"] == KERNEL
    assert plan(tc.over_program(100000, np.float64, np.float64), np.float64)["kernel"] == KERNEL
    for mode in tc.MODES:
        assert plan(tc.multi_program(64, 2, mode=mode))["kernel"] == KERNEL


def test_any_other_program_with_either_op_is_refused_by_name():
    shape = ("DSP_OP_MULTI_TIME_POINT_THRESH / DSP_OP_TIME_OVER_THRESHOLD.*multi_time_point_thresh, time_over_threshold.*dsp_thresh_kernel only"
             ".*LOAD, \\[LOAD of the thresholds,\\] MULTI_TIME_POINT_THRESH, STORE; or LOAD, TIME_OVER_THRESHOLD, STORE_SCALAR")
    p = tc.multi_program(1000, 3)
    p.ops.pop()  # no store
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = tc.multi_program(1000, 3)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = tc.over_program(1000)
    p.n_sregs = 5
    p.add_op(_lib.OP_MIN_MAX, dst=1, src=0)  # no fusion with min_max
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = tc.over_program(1000)  # both ops in one program
    p.slots.append(3)
    p.ops.insert(2, (_lib.OP_MULTI_TIME_POINT_THRESH, 1, 0, p.add_io("thr", _lib.IO_TAPS, np.float32, 3), (ord("l"), -1), (Scalar.const(0.0), Scalar.const(1.0))))
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    with pytest.raises(NotImplementedError, match="the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
        plan(tc.multi_program(1000, 3, np.int32, np.float64), np.float64)
    with pytest.raises(NotImplementedError, match="the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
        plan(tc.over_program(1000, np.uint32, np.float64), np.float64)
    p = tc.multi_program(1000, 3)
    op = list(p.ops[1])
    op[5] = (Scalar.reg(0), Scalar.const(1.0))
    p.ops[1], p.n_sregs = tuple(op), 1
    with pytest.raises(NotImplementedError, match="t_start is a constant or a per-event column of the loop's type"):
        plan(p)
    p = tc.multi_program(1000, 3)
    op = list(p.ops[1])
    op[3] = 0  # the rows' binding where the list's should be
    p.ops[1] = tuple(op)
    with pytest.raises(NotImplementedError, match="the thresholds are one list for every row .*or a list per row"):
        plan(p)
    p = tc.over_program(1000)
    op = list(p.ops[1])
    op[5] = (Scalar.reg(0),)
    p.ops[1] = tuple(op)
    with pytest.raises(NotImplementedError, match="the threshold is a constant or a per-event column of the loop's type"):
        plan(p)


def test_the_reference_s_checks_and_the_bounds():
    for pol in (0.0, -0.0, np.nan):
        with pytest.raises(DSPFatal, match="polarity cannot be 0"):
            plan(tc.multi_program(1000, 3, polarity=pol))
    for mode in ("h", "s", "x", "L"):
        with pytest.raises(DSPFatal, match="Unrecognized interpolation mode"):
            plan(tc.multi_program(1000, 3, mode=mode))
    with pytest.raises(NotImplementedError, match="the polarity is a constant of the program, not a per-event value"):
        plan(tc.multi_program(1000, 3, polarity="column"))
    plan(tc.multi_program(1000, tc.THRESH_MAX))
    with pytest.raises(NotImplementedError, match="multi_time_point_thresh: at most 64 thresholds \\(65 given\\)"):
        plan(tc.multi_program(1000, tc.THRESH_MAX + 1))
    with pytest.raises(NotImplementedError, match="multi_time_point_thresh: rows of at least 2 samples"):
        plan(tc.multi_program(1, 3))
    p = tc.multi_program(1000, 3)
    p.io[1] = p.io[1][:3] + (4,) + p.io[1][4:]  # four thresholds for three times
    with pytest.raises(ValueError, match="writes a time per threshold \\(4 thresholds, 3 times\\)"):
        plan(p)
    with pytest.raises(ValueError, match="at most 2\\^20 samples"):  # (every slot's bound, well inside the 2^24 a float32 time counts exactly)
        plan(tc.multi_program((1 << 20) + 1, 3))


def test_registry_abi_and_messages():
    from dspeed_amd import processors

    assert "multi_time_point_thresh" in processors.__all__ and "time_over_threshold" in processors.__all__
    g = processors.multi_time_point_thresh
    assert g.signature == "(n),(m),(),(),()->(m)" and g.types == ["ffffb->f", "ddddb->d"] and (g.nin, g.nout) == (5, 1)
    g = processors.time_over_threshold
    assert g.signature == "(n),()->()" and g.types == ["ff->f", "dd->d"] and (g.nin, g.nout) == (2, 1)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, f"dsp_{name}_{sfx}") for name in ("multi_time_point_thresh", "time_over_threshold") for sfx in ("f32", "f64"))
    assert (_lib.OP_MULTI_TIME_POINT_THRESH, _lib.OP_TIME_OVER_THRESHOLD, _lib.THRESH_MAX) == (37, 38, 64)
    L.dsp_fatal_message.restype = ctypes.c_char_p
    assert [L.dsp_fatal_message(c).decode() for c in (31, 32)] == ["polarity cannot be 0", "Unrecognized interpolation mode"]
    from dspeed_amd.language import module_accepted

    assert module_accepted(f"{M}.time_point_thresh", "multi_time_point_thresh") and module_accepted(f"{M}.time_over_threshold", "time_over_threshold")
    assert module_accepted(M, "multi_time_point_thresh") and not module_accepted(f"{M}.time_point_thresh", "time_over_threshold")


def test_the_host_checks_raise_with_the_reference_s_texts():
    """polarity and mode are constants of the call: checked before anything is sent to a device, for every row"""
    from dspeed_amd.processors import multi_time_point_thresh

    w, thr = np.full((4, 10), np.nan, dtype=np.float32), np.float32([1, 2])  # (NaN rows: the reference would return before its checks)
    with pytest.raises(DSPFatal, match="polarity cannot be 0"):
        multi_time_point_thresh(w, thr, 5, 0, "l")
    with pytest.raises(DSPFatal, match="Unrecognized interpolation mode"):
        multi_time_point_thresh(w, thr, 5, 1, ord("h"))
    with pytest.raises(NotImplementedError, match="polarity is a constant of the call"):
        multi_time_point_thresh(w, thr, 5, np.float32([1, 1, -1, 1]), "l")
    with pytest.raises(NotImplementedError, match="mode_in is a constant of the call"):
        multi_time_point_thresh(w, thr, 5, 1, np.array([ord("l")] * 4, dtype=np.int8))


def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def test_a_rise_time_recipe_builds_one_stage_for_each_processor(monkeypatch):
    from dspeed_amd.processing_chain import build_processing_chain

    rng = np.random.default_rng(5)
    tb = {"waveform": tc.recipe_rows()[:12], "bl": rng.uniform(990, 1010, 12).astype(np.float32)}
    chain, _, out = build_processing_chain({"outputs": ["tps", "t_sat"], "processors": tc.rise_time_recipe()}, tb)
    stages = _stages(chain)
    mine = [s for s in stages if s[1] == KERNEL]
    assert [s[2] for s in mine] == [[_lib.OP_LOAD, _lib.OP_MULTI_TIME_POINT_THRESH, _lib.OP_STORE], [_lib.OP_LOAD, _lib.OP_TIME_OVER_THRESHOLD, _lib.OP_STORE_SCALAR]]
    assert mine[0][0] == "multi_time_point_thresh tps on rows" and mine[1][0] == "time_over_threshold t_sat on rows"
    whats = [s[0] for s in stages]
    # the sources are not rows in memory: each is written there ahead of its stage
    assert whats.index("wf_norm -> HBM") < whats.index(mine[0][0]) and whats.index("wf_blsub -> HBM") < whats.index(mine[1][0])
    assert whats.index("per-event values of wf_blsub") < whats.index(mine[1][0])  # (min_max moves ahead: it reads rows in memory now)
    assert out["tps"].shape == (12, 3) and out["tps"].dtype == np.float32 and out["t_sat"].shape == (12,)
    # a threshold read off a waveform the program computes, for a stage on the input rows: written to memory with its processor's other results
    chain, _, out = build_processing_chain({"outputs": ["n_over", "wf_max", "tp_max"], "processors": tc.over_half_recipe()}, tb)
    whats = [s[0] for s in _stages(chain)]
    assert whats.index("wf_max -> HBM") < whats.index("time_over_threshold n_over on rows") and not any(w.startswith("waveform ->") for w in whats)
    # rows that are chain inputs are read as they are; a list per event is a two-dimensional input column
    tb2 = {"waveform": tb["waveform"], "lists": np.tile(np.float32([1100, 1500]), (12, 1)), "start": np.full(12, 400, np.float32)}
    procs = {"tps": {"function": "multi_time_point_thresh", "module": M, "args": ["waveform", "lists", "start", -1, "'n'", "tps"]},
             "n_over": {"function": "time_over_threshold", "module": M, "args": ["waveform", 1200, "n_over"]}}
    chain, _, out = build_processing_chain({"outputs": ["tps", "n_over"], "processors": procs}, tb2)
    stages = _stages(chain)
    assert [s[2] for s in stages if s[1] == KERNEL] == [[_lib.OP_LOAD, _lib.OP_LOAD, _lib.OP_MULTI_TIME_POINT_THRESH, _lib.OP_STORE],
                                                        [_lib.OP_LOAD, _lib.OP_TIME_OVER_THRESHOLD, _lib.OP_STORE_SCALAR]]
    assert not any("-> HBM" in s[0] for s in stages) and out["tps"].shape == (12, 2)

    def build(args, table=tb2, fn="multi_time_point_thresh"):
        return build_processing_chain({"outputs": ["tps"], "processors": {"tps": {"function": fn, "module": M, "args": args}}}, table)

    # refusals, by name
    with pytest.raises(DSPFatal, match="polarity cannot be 0"):
        build(["waveform", "[1100, 1500]", 400, 0, "'l'", "tps"])
    with pytest.raises(DSPFatal, match="Unrecognized interpolation mode"):
        build(["waveform", "[1100, 1500]", 400, 1, "'h'", "tps"])
    with pytest.raises(NotImplementedError, match="multi_time_point_thresh \\(tps\\): at most 64 thresholds \\(65 given\\)"):
        build(["waveform", str(list(range(65))), 400, 1, "'l'", "tps"])
    with pytest.raises(NotImplementedError, match="the polarity is a constant of the kernel, not a per-event value"):
        build(["waveform", "[1100, 1500]", 400, "start", "'l'", "tps"])
    with pytest.raises(NotImplementedError, match="the interpolation mode is a constant of the kernel, not a per-event value"):
        build(["waveform", "[1100, 1500]", 400, 1, "start", "tps"])
    with pytest.raises(NotImplementedError, match="a threshold list computed per event inside the recipe is not supported"):
        build(["waveform", "lists*2", 400, 1, "'l'", "tps"])
    for fn, args in (("multi_time_point_thresh", ["waveform", "[1100.0, 1500.0]", 400, 1, "'l'", "tps"]), ("time_over_threshold", ["waveform", 1200, "tps"])):
        with pytest.raises(NotImplementedError, match=f"{fn} in a recipe whose loop type is float64"):
            build(args, {"waveform": tb["waveform"].astype(np.float64)}, fn)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    for fn, args in (("multi_time_point_thresh", ["waveform", "[1100, 1500]", 400, 1, "'l'", "tps"]), ("time_over_threshold", ["waveform", 1200, "tps"])):
        with pytest.raises(NotImplementedError, match=f"{fn}.*DSPEED_HIP_NO_STAGES"):
            build(args, fn=fn)
