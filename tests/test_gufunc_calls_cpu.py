"""The Python half of a gufunc call on the CPU: what ``HipGUFunc.__call__`` hands to the library.

Every device-backed processor of ``dspeed_amd.processors`` is called against ``tests/fake_dsp_lib.py`` -- 1-D and 2-D rows, int16 / float32 /
float64 rows, each ``()`` argument as a Python scalar, a 0-d array, a length-1 array and one value per row, outputs passed and omitted, rows,
columns and outputs on the "device" -- and the recorded entry-point calls (name, argument order, which pointer is which allocation, every
scalar as converted), the shape of what comes back, or the exception's type and text, are compared with ``tests/golden/gufunc_calls.json.gz``,
EXACTLY.  The fixture was recorded (``tools/record_gufunc_calls.py``) from the hand-written implementations, one per processor, before they
became descriptions for one generic frame.  What it holds is what those did, their one slip included: a ``level`` per row for
``discrete_wavelet_transform`` ends in an IndexError in ``HipGUFunc._by_parameter_value``, which keeps no result list for a gufunc whose
outputs are all in place."""
import gzip
import json
import os

import numpy as np
import pytest

import fake_dsp_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gufunc_calls.json.gz")
N_WF, LEN = 3, 16

# name: (inputs after the rows, outputs).  An output is "" (a value per row), "n" (a row of the input's length) or a length m; a length
# stands for an output that has to be passed.  None of the values is a float32, so that a conversion through the loop's type shows.
#                                          inputs                            outputs
PROCESSORS = {
    "bl_subtract":                        ([1.1],                            ["n"]),
    "pole_zero":                          ([100.3],                          ["n"]),
    "double_pole_zero":                   ([100.3, 10.7, 0.3],               ["n"]),
    "trap_filter":                        ([4, 2],                           ["n"]),
    "trap_norm":                          ([4, 2],                           ["n"]),
    "asym_trap_filter":                   ([4, 2, 3],                        ["n"]),
    "fixed_time_pickoff":                 ([7.3, "i"],                       [""]),
    "time_point_thresh":                  ([0.7, 12.0, 1.0],                 [""]),
    "interpolated_time_point_thresh":     ([0.7, 12.0, 1, "l"],              [""]),
    "min_max":                            ([],                               ["", "", "", ""]),
    "min_max_norm":                       ([-2.1, 3.3],                      ["n"]),
    "linear_slope_fit":                   ([],                               ["", "", "", ""]),
    "mean_below_threshold":               ([0.7],                            [""]),
    "windower":                           ([3.3],                            [8]),
    "avg_current":                        ([10.1],                           [6]),
    "upsampler":                          ([0.3],                            [8]),
    "moving_window_multi":                ([3.1, 2.0, 1],                    ["n"]),
    "trap_pickoff":                       ([4, 2, 11.3],                     [""]),
    "discrete_wavelet_transform":         ([1, "h", "a"],                    [8]),
    "convolve_wf":                        (["taps", "v"],                    [13]),
    "fft_convolve_wf":                    (["taps", "f"],                    [19]),
    "get_multi_local_extrema":            ([0.7, 0.3, 3, 1.1, -1.1],         [5, 5, "", ""]),
    "histogram":                          ([],                               [4, 5]),
    "multi_time_point_thresh":            (["thresholds", 6.3, -1.1, "i"],   ["m"]),
    "time_over_threshold":                ([0.7],                            [""]),
}
COLUMNS = {"bl_subtract": [0], "pole_zero": [0], "double_pole_zero": [0, 1, 2], "fixed_time_pickoff": [0], "time_point_thresh": [0, 1],
           "interpolated_time_point_thresh": [0, 1], "min_max_norm": [0, 1], "mean_below_threshold": [0], "windower": [0], "trap_pickoff": [2],
           "get_multi_local_extrema": [0, 1, 3, 4], "multi_time_point_thresh": [1], "time_over_threshold": [0], "histogram_stats": [0]}
HOST_ONLY = {"cusp_filter", "zac_filter", "t0_filter", "moving_slope"}  # kernel generators: NumPy, no library call
TAPS = [1.0, -0.5, 0.3, 2.0]
THRESHOLDS = [0.1, 0.2, 0.3, 0.4]
ROW_KINDS = {"1d-f32": ((LEN,), np.float32), "f32": ((N_WF, LEN), np.float32), "i16": ((N_WF, LEN), np.int16), "f64": ((N_WF, LEN), np.float64)}
SPELLINGS = ("scalar", "0d", "len1", "per-row")


def _loop_type(dtype):
    return np.float32 if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.int16)) else np.float64


def _spell(value, how, n_wf):
    if isinstance(value, list):  # (the values of the rows, spelled out)
        return np.array(value)
    if how == "scalar":
        return value
    if how == "0d":
        return np.array(value)
    return np.array([value] * (1 if how == "len1" else n_wf))


def _rows(kind, width=LEN):
    shape, dtype = ROW_KINDS[kind]
    shape = shape[:-1] + (width,)
    return (np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)


class Case:
    """one call: the processor, how its rows, inputs and outputs are given; ``device``: names of arguments handed over as DeviceArrays"""

    def __init__(self, name, rows="f32", spell=None, outs="omitted", device=(), **changes):
        self.name, self.rows, self.spell, self.outs, self.device, self.changes = name, rows, spell or {}, outs, device, changes
        self.id = "-".join([name, rows] + [f"arg{k}:{how}" for k, how in sorted(self.spell.items())] + [f"outs:{outs}"] + [f"dev:{d}" for d in device] +
                           [f"{k}={v}" for k, v in sorted(changes.items())])

    def arguments(self, made):
        """(processor, positional arguments); DeviceArrays made on the way are appended to ``made``"""
        from dspeed_amd import processors
        from dspeed_amd.device import DeviceArray

        def dev(a):
            made.append(DeviceArray.from_numpy(a))
            return made[-1]

        if self.name == "histogram_stats":
            return getattr(processors, self.name), self._histogram_stats(dev)
        inputs, outputs = PROCESSORS[self.name]
        rows = _rows(self.rows)
        ft = _loop_type(rows.dtype)
        lead = rows.shape[:-1]
        n_wf = rows.shape[0] if rows.ndim == 2 else 1
        args = [dev(rows) if "rows" in self.device else rows]
        for k, v in enumerate(inputs):
            if v == "taps":
                v = np.asarray(self.changes.get("taps", TAPS), dtype=ft)
                v = dev(v) if "taps" in self.device else v
            elif v == "thresholds":
                v = np.asarray(self.changes.get("thresholds", THRESHOLDS), dtype=self.changes.get("thresholds_dtype", ft))
                v = np.tile(v, (n_wf, 1)) if self.changes.get("thresholds_per_row") else v
                v = dev(v) if "thresholds" in self.device else v
            else:
                v = _spell(self.changes.get(f"arg{k}", v), self.spell.get(k, "scalar"), n_wf)
                if f"arg{k}" in self.device:
                    v = dev(np.full(n_wf, v, dtype=self.changes.get("column_dtype", ft)))
            args.append(v)
        m = len(self.changes.get("thresholds", THRESHOLDS))
        given = []
        for k, o in enumerate(outputs):
            shape = lead + {"": (), "n": (LEN,), "m": (m,)}.get(o, (o,))
            dtype = np.uint32 if self.name == "get_multi_local_extrema" and k >= 2 else ft
            if self.outs == "omitted" and not isinstance(o, int):
                continue
            if self.outs == "none-passed":
                continue
            if self.outs == "wrong-shape":
                shape = shape[:-1] + (shape[-1] + 1,) if shape else (2,)
            a = np.zeros(shape, dtype=dtype)
            given.append(dev(a) if "outs" in self.device else a)
        return getattr(processors, self.name), args + given

    def _histogram_stats(self, dev):
        weights, edges = _rows(self.rows, 4), _rows(self.rows, self.changes.get("edges", 5))
        ft = _loop_type(weights.dtype)
        n_wf = weights.shape[0] if weights.ndim == 2 else 1
        if self.changes.get("edges_rows"):
            edges = edges[: self.changes["edges_rows"]]
        if self.changes.get("edges_dtype"):
            edges = edges.astype(self.changes["edges_dtype"])
        max_in = _spell(self.changes.get("arg0", 2.3), self.spell.get(0, "scalar"), n_wf)
        if "arg0" in self.device:
            max_in = dev(np.full(n_wf, max_in, dtype=ft))
        outs = [None] * 3 if self.outs == "omitted" else [np.zeros(weights.shape[:-1], dtype=ft) for _ in range(3)]
        if "rows" in self.device:
            weights, edges = dev(weights), dev(edges)
        if self.outs == "none-passed":
            return [weights, edges, max_in]
        return [weights, edges, *outs, max_in]


def _cases():
    cases = []
    for name, (inputs, outputs) in list(PROCESSORS.items()) + [("histogram_stats", ([2.3], ["", "", ""]))]:
        scalars = [k for k, v in enumerate(inputs) if v not in ("taps", "thresholds")]
        for rows in ROW_KINDS:
            for outs in ("omitted", "passed"):
                cases.append(Case(name, rows, outs=outs))
        for k in scalars:  # each () argument in each spelling, beside Python scalars
            for how in SPELLINGS[1:]:
                cases.append(Case(name, "f32", {k: how}))
            cases.append(Case(name, "1d-f32", {k: "per-row"}))
            if k in COLUMNS.get(name, ()):  # (an argument the kernels read as a column)
                cases.append(Case(name, "f32", device=(f"arg{k}",)))
                cases.append(Case(name, "f64", device=(f"arg{k}",), column_dtype="float32"))  # a column of the other loop's type
        cases.append(Case(name, "f32", outs="passed", device=("rows", "outs")))
        cases.append(Case(name, "f64", outs="passed", device=("rows",)))
        cases.append(Case(name, "f32", outs="wrong-shape"))
        if any(isinstance(o, int) for o in outputs) or name == "histogram_stats":
            cases.append(Case(name, "f32", outs="none-passed"))
    cases += [
        Case("trap_filter", "f32", {0: "per-row"}, arg0=[4, 5, 4]),  # rows grouped by parameter value: two launches
        Case("trap_filter", "f32", {0: "per-row", 1: "per-row"}, outs="passed", arg0=[4, 5, 4], arg1=[2, 2, 1]),
        Case("trap_filter", "f32", {0: "per-row"}, arg0=[4, float("nan"), 4]),
        Case("trap_filter", "f32", arg0=float("nan")),
        Case("trap_filter", "f32", {0: "per-row"}, device=("rows",), arg0=[4, 5, 4]),
        Case("asym_trap_filter", "f64", {2: "per-row"}, arg2=[3, 1, 3]),
        Case("moving_window_multi", "f32", {2: "per-row"}, arg2=[0, 1, 0]),
        Case("discrete_wavelet_transform", "f32", arg1="x"),  # not the Haar wavelet
        Case("discrete_wavelet_transform", "f32", arg1="d", arg2="d"),
        Case("fixed_time_pickoff", "f32", arg1=np.array("n")),
        Case("fixed_time_pickoff", "f32", arg1=np.int8(ord("l"))),
        Case("convolve_wf", "f32", device=("taps",)),
        Case("convolve_wf", "f64", device=("taps",), outs="passed"),
        Case("convolve_wf", "f32", taps=[[1.0, 2.0], [3.0, 4.0]]),  # a kernel per row
        Case("multi_time_point_thresh", "f32", thresholds_per_row=True),
        Case("multi_time_point_thresh", "f64", thresholds_per_row=True, outs="passed"),
        Case("multi_time_point_thresh", "f32", device=("thresholds",)),
        Case("multi_time_point_thresh", "f32", device=("thresholds",), thresholds_per_row=True),
        Case("multi_time_point_thresh", "f32", device=("thresholds",), thresholds_dtype="float64"),
        Case("multi_time_point_thresh", "f32", thresholds=[]),
        Case("multi_time_point_thresh", "f32", thresholds=[], outs="passed"),
        Case("multi_time_point_thresh", "f32", thresholds=[0.5] * 65),
        Case("multi_time_point_thresh", "f32", thresholds=[[[0.5]]]),
        Case("multi_time_point_thresh", "f32", arg2=0.0),
        Case("multi_time_point_thresh", "f32", arg2=float("nan")),
        Case("multi_time_point_thresh", "f32", arg3="x"),
        Case("multi_time_point_thresh", "f32", arg3=200),
        Case("histogram_stats", "f32", edges_rows=2),
        Case("histogram_stats", "f32", edges_dtype="float64"),
    ]
    return cases


CASES = _cases()


def record(case):
    """what the call hands to the library and what it gives back, as JSON holds it"""
    from dspeed_amd.device import DeviceArray

    def describe(r, args):
        if isinstance(r, tuple):
            return [describe(x, args) for x in r]
        same = [k for k, a in enumerate(args) if a is r]
        kind = type(r).__name__ if isinstance(r, (np.ndarray, DeviceArray)) else "scalar"
        return [kind, str(np.asarray(r).dtype) if kind == "scalar" else str(r.dtype), list(np.shape(r) if kind == "scalar" else r.shape)] + same

    made = []
    with fake_dsp_lib.installed() as fake:
        try:
            fn, args = case.arguments(made)
            try:
                out = {"result": describe(fn(*args), args)}
            except Exception as e:  # noqa: BLE001 -- (type and text are what is recorded)
                out = {"raises": [type(e).__name__, str(e)]}
            out["calls"] = fake.calls
            out["live"] = fake.live() - len(made)  # device memory of the call itself still allocated after it
        finally:
            for d in made:
                d.free()
    return json.loads(json.dumps(out))


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def test_the_cases_cover_every_device_backed_processor(golden):
    from dspeed_amd import processors

    assert {c.name for c in CASES} == set(processors.__all__) - HOST_ONLY
    assert len({c.id for c in CASES}) == len(CASES)
    assert sorted(golden) == sorted(c.id for c in CASES)


@pytest.mark.parametrize("name", sorted({c.name for c in CASES}))
def test_calls_are_the_recorded_ones(golden, name):
    for case in CASES:
        if case.name == name:
            got = record(case)
            assert got == golden[case.id], case.id
            assert got["live"] == 0, case.id  # (whatever the call raised)


def _raised(golden, case):
    assert record(case) == golden[case.id]
    return tuple(golden[case.id]["raises"])


def test_documented_refusals_keep_type_and_text(golden):
    """the exceptions of the implementations, by type and text (each case is also in the fixture)"""
    for name, text in (("windower", "windower(w_in, t0_in, w_out): w_out must be passed (its length is the window size)"),
                       ("avg_current", "avg_current(w_in, length, w_out): w_out must be passed (len(w_in) - int(length) samples)"),
                       ("upsampler", "upsampler(w_in, upsample, w_out): w_out must be passed (its length is the output size)"),
                       ("histogram", "histogram(w_in, weights_out, borders_out): both outputs must be passed (len(weights_out) is the number of bins)"),
                       ("discrete_wavelet_transform", "discrete_wavelet_transform(w_in, level, wave_type, coeff, w_out): w_out must be passed (its length is the output size)"),
                       ("convolve_wf", "convolve_wf(w_in, kernel, mode_in, w_out): w_out must be passed (its length selects the output size)"),
                       ("fft_convolve_wf", "fft_convolve_wf(w_in, kernel, mode_in, w_out): w_out must be passed (its length selects the output size)")):
        assert _raised(golden, Case(name, "f32", outs="none-passed")) == ("TypeError", text)
    assert _raised(golden, Case("get_multi_local_extrema", "f32", outs="none-passed"))[1].endswith(
        "vt_max_out and vt_min_out must be passed (their length is the number of extrema kept)")
    assert _raised(golden, Case("histogram_stats", "f32", outs="none-passed"))[1].endswith("pass None to have them allocated")
    assert _raised(golden, Case("bl_subtract", "f32", outs="wrong-shape")) == ("ValueError", "Outputs are not the right shape")
    assert _raised(golden, Case("bl_subtract", "f64", device=("arg0",), column_dtype="float32")) == ("TypeError", "per-waveform scalar column must be float64")
    assert _raised(golden, Case("trap_filter", "f32", arg0=float("nan"))) == ("NotImplementedError", "trap_filter: NaN integer parameter")
    assert _raised(golden, Case("trap_filter", "f32", {0: "per-row"}, arg0=[4, float("nan"), 4])) == ("NotImplementedError", "trap_filter: NaN integer parameter")
    assert _raised(golden, Case("trap_filter", "f32", {0: "per-row"}, device=("rows",), arg0=[4, 5, 4])) == (
        "NotImplementedError", "trap_filter: per-waveform integer parameters need the rows in host memory (they are grouped by value)")
    assert _raised(golden, Case("discrete_wavelet_transform", "f32", arg1="x")) == ("NotImplementedError", "only the Haar wavelet ('h' / 'd' = db1) is implemented")
    assert _raised(golden, Case("convolve_wf", "f32", taps=[[1.0, 2.0], [3.0, 4.0]])) == ("NotImplementedError", "per-waveform kernels are not supported")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", arg2=0.0)) == ("DSPFatal", "polarity cannot be 0")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", arg2=float("nan"))) == ("DSPFatal", "polarity cannot be 0")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", arg3="x")) == ("DSPFatal", "Unrecognized interpolation mode")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", arg3=200)) == ("DSPFatal", "Unrecognized interpolation mode")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", thresholds=[0.5] * 65)) == (
        "NotImplementedError", "multi_time_point_thresh: at most 64 thresholds (65 given): a wavefront keeps one per lane")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", thresholds=[[[0.5]]])) == (
        "ValueError", "multi_time_point_thresh: a_threshold has shape (1, 1, 1), expected (m,) or (3, m)")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", device=("thresholds",), thresholds_dtype="float64")) == (
        "TypeError", "multi_time_point_thresh: thresholds on the device have the loop's type, float32")
    assert _raised(golden, Case("multi_time_point_thresh", "f32", {2: "per-row"})) == (
        "NotImplementedError", "multi_time_point_thresh: polarity is a constant of the call on the device, not a per-event value")
    assert _raised(golden, Case("histogram_stats", "i16")) == (
        "TypeError", "histogram_stats: weights_in and edges_in are float32 (the float32 loop) or float64 rows of one type")
    assert _raised(golden, Case("histogram_stats", "f32", edges_rows=2)) == ("ValueError", "histogram_stats: weights_in and edges_in hold the same number of rows")
    for name in ("histogram", "time_over_threshold", "multi_time_point_thresh"):  # the float64 loop of these takes float64 rows only
        rows = np.zeros((N_WF, LEN), dtype=np.int32)
        fn, args = Case(name, "f32", outs="passed").arguments([])
        with fake_dsp_lib.installed() as fake, pytest.raises(NotImplementedError, match=f"^{name}: the float64 loop takes float64 rows on the device$"):
            fn(rows, *args[1:])
        assert fake.calls == [] and fake.live() == 0


def test_the_stand_in_is_taken_out_again():
    from dspeed_amd import _lib, device

    before = _lib._lib
    with fake_dsp_lib.installed() as fake:
        assert _lib.lib() is fake
        device.DeviceArray.from_numpy(np.arange(4.0)).free()  # (makes the bounce buffer)
        assert "buf" in device._Bounce._local.__dict__ and fake.host
    assert _lib._lib is before and not fake.host
