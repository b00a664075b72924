"""The planner's, the registry's and the recipe compiler's part of reflected_convolve_wf without a device (dsp_chain_plan):
DSP_OP_REFLECTED_CONVOLVE has one route -- dsp_reflect_kernel, whatever the switches say --, two program shapes (alone, and with an
avg_current of the filtered row in the same launch) and every refusal by name; the opcode is appended; the two processors are attributes of
the registry listed in ``SMOOTHING``; what a call hands to the library (against a subclass of tests/fake_dsp_lib.FakeLib); the stage list of
the SiPM fragment behind the filter."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import fake_dsp_lib
import histogram_cases as hc
import reflect_cases as rc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import DSPFatal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = rc.KERNEL
F64 = dict(rows=np.float64, loop=np.float64)
L, RC, AC, ST = _lib.OP_LOAD, _lib.OP_REFLECTED_CONVOLVE, _lib.OP_AVG_CURRENT, _lib.OP_STORE


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_both_shapes_take_the_reflect_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for n, m in rc.pairs("f32"):
            assert plan(rc.program(n, m))["kernel"] == KERNEL
        for n, m in rc.pairs("f64"):
            assert plan(rc.program(n, m, **F64), np.float64)["kernel"] == KERNEL
        for rows in (np.int16, np.uint16):
            assert plan(rc.program(1000, 9, rows))["kernel"] == KERNEL
            assert plan(rc.program(1000, 9, rows, offset=3, row_stride=1007, out_stride=1005))["kernel"] == KERNEL
        for lag in (5, 1):
            for store_row in (True, False):
                assert plan(rc.program(1000, 9, lag=lag, store_row=store_row))["kernel"] == KERNEL
                assert plan(rc.program(4096, 65, lag=lag, store_row=store_row, **F64), np.float64)["kernel"] == KERNEL
        assert plan(rc.program(1000, 9, lag=5, length=5.5))["kernel"] == KERNEL  # (int(length) samples apart, divided by length)

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_geometry_the_case_book_assumes_is_the_headers():
    kernels_h = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    mine = kernels_h[kernels_h.index("namespace dsp_reflect {"):kernels_h.index("}  // namespace dsp_reflect")]
    assert "constexpr int WAVE_ROW_BYTES = 8 * 1024, LDS_MAX = 64 * 1024;" in mine and "F32_MAX = LDS_MAX / 4, F64_MAX = LDS_MAX / 8" in mine
    assert rc.T * 4 == 8 * 1024 and rc.F32_MAX * 4 == 64 * 1024 == rc.F64_MAX * 8


def test_the_limits_by_name():
    assert (_lib.REFLECT_F32_MAX, _lib.REFLECT_F64_MAX) == (rc.F32_MAX, rc.F64_MAX) == (16384, 8192)
    header = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_program.h")).read()
    assert "#define DSP_REFLECT_F32_MAX 16384" in header and "#define DSP_REFLECT_F64_MAX 8192" in header
    for rows, kw, loop in (("f32", {}, np.float32), ("f64", F64, np.float64)):
        for n, m in rc.over_the_limit(rows):
            with pytest.raises(NotImplementedError, match=f"reflected_convolve_wf: {rc.LIMITS} \\(len\\(w_in\\) = {n}, len\\(kernel\\) = {m} given\\): "
                                                          "a row and its mirrored margins live in 64 KiB of LDS"):
                plan(rc.program(n, m, **kw), loop)
    with pytest.raises(NotImplementedError, match=f"reflected_convolve_wf: {rc.LIMITS}"):
        plan(rc.program(1 << 19, 3))


def test_a_kernel_longer_than_the_rows_is_an_argument_error_in_the_references_words():
    for n, m in ((8, 9), (1, 2), (1000, 1001)):
        with pytest.raises(ValueError, match=f"The filter is longer than the input waveform \\({m} taps, {n} samples\\)"):
            plan(rc.program(n, m))
        with pytest.raises(ValueError, match="The filter is longer than the input waveform"):
            plan(rc.program(n, m, **F64), np.float64)


def test_any_other_program_with_the_op_is_refused_by_name():
    shape = ("DSP_OP_REFLECTED_CONVOLVE \\(reflected_convolve_wf\\) runs on dsp_reflect_kernel only, on rows in memory: the program must be exactly "
             "LOAD, REFLECTED_CONVOLVE, STORE; or LOAD, REFLECTED_CONVOLVE, AVG_CURRENT, STORE \\[, STORE\\]")
    p = rc.program(1000, 9)
    p.ops.pop()  # no store
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = rc.program(1000, 9)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = rc.program(1000, 9)
    p.n_sregs = 4
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=1)  # a second reader of the filtered row
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = rc.program(1000, 9, lag=5)
    p.add_op(ST, src=2, io=p.add_io("curr2", _lib.IO_WF_OUT, np.float32, 995, 0, None))  # the current stored twice
    with pytest.raises(NotImplementedError, match="DSP_OP_REFLECTED_CONVOLVE.*(the program must be exactly|the current is stored once)"):
        plan(p)
    p = rc.program(1000, 9, lag=5)
    p.ops[2] = p.ops[2][:2] + (0,) + p.ops[2][3:]  # an avg_current of the raw row, not of the filtered one
    with pytest.raises(NotImplementedError, match="DSP_OP_REFLECTED_CONVOLVE.*the avg_current in the same program reads exactly the filtered row"):
        plan(p)
    p = rc.program(1000, 9, lag=5, store_row=False)
    p.ops.pop()  # a fused program that stores nothing
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = rc.program(1000, 9)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # destination = source
    with pytest.raises(ValueError, match="bad REFLECTED_CONVOLVE \\(src: the slot of the row; dst: another slot, for the filtered row"):
        plan(p)
    for out_len in (999, 1001, 1):  # an output whose length is not the input's: an argument error that names both
        with pytest.raises(ValueError, match=f"reflected_convolve_wf: the output has the length of the input \\(len\\(w_in\\) = 1000, len\\(w_out\\) = {out_len}\\)"):
            plan(rc.program(1000, 9, out_len=out_len))
    for rows in (np.int32, np.uint32):
        with pytest.raises(NotImplementedError, match="DSP_OP_REFLECTED_CONVOLVE.*the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(rc.program(1000, 9, rows, np.float64), np.float64)
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(rc.program(1000, 9, np.float64, np.float32))


def test_the_opcode_is_appended_and_the_registry_lists_the_processors_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _GENERATORS, _PROCESSOR_FILES, module_accepted

    assert (_lib.OP_DENSE, _lib.OP_REFLECTED_CONVOLVE) == (44, 45)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_REFLECTED_CONVOLVE 45" in header and "#define DSP_OP_DENSE 44" in header
    assert "dsp_reflected_convolve_f32" not in header and "dsp_reflected_convolve_f64" not in header  # (one entry, the loop an argument)
    assert processors.SMOOTHING == ("reflected_convolve_wf", "gaussian_filter1d")
    others = set(processors.__all__) | set(processors.SPECTRAL) | set(processors.ORDER) | set(processors.RESAMPLING) | set(processors.ML) | set(_PROCESSOR_FILES)
    assert not set(processors.SMOOTHING) & others and "gaussian_filter1d" not in _GENERATORS
    g = processors.reflected_convolve_wf
    assert g.signature == "(n),(m),(p)" and g.types == ["fff", "ddd"] and g.nargs == 3 and g.__name__ == "reflected_convolve_wf"
    g = processors.gaussian_filter1d
    assert g.signature == "(),(),(n)" and g.types == ["fff", "ddd"] and g.nargs == 3 and g.__name__ == "gaussian_filter1d"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dsp_reflected_convolve_rows") and "dsp_reflected_convolve_rows" in _lib.EXPORTS
    fn = "reflected_convolve_wf"
    assert module_accepted(M, fn) and module_accepted(f"{M}.convolutions", fn) and module_accepted("dspeed_amd.processors", fn)
    assert not module_accepted(f"{M}.fft", fn) and not module_accepted(f"{M}.gaussian_filter1d", fn)


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entry that names its loop in an argument instead of a suffix"""

    def dsp_reflected_convolve_rows(self, *args):
        self.calls.append(["dsp_reflected_convolve_rows"] + [self._name(a) for a in args])
        return 0


@contextlib.contextmanager
def _installed():
    from dspeed_amd import device

    real, bounce = _lib._lib, device._Bounce._local.__dict__.pop("buf", None)
    fake = _Fake(real)
    _lib._lib = fake
    try:
        yield fake
    finally:
        device._Bounce._local.__dict__.pop("buf", None)
        if bounce is not None:
            device._Bounce._local.buf = bounce
        _lib._lib = real


N_WF, LEN, TAPS = 3, 16, 5


def _rows(dtype, shape=(N_WF, LEN)):
    return (np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)


@pytest.mark.parametrize("dtype, code, loop_code, loop", [(np.float32, _lib.F32, _lib.F32, np.float32), (np.int16, _lib.I16, _lib.F32, np.float32),
                                                          (np.uint16, _lib.U16, _lib.F32, np.float32), (np.float64, _lib.F64, _lib.F64, np.float64)])
def test_the_arguments_of_a_call(dtype, code, loop_code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, the kernel (pointer, taps), the output and its stride, the stream, the
    row of an error"""
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    k = np.arange(TAPS, dtype=np.float64)  # (a host kernel of any number type: converted to the loop's)
    with _installed() as fake:
        # a 2-D call, the output left out: a new array of the loop's type
        r = processors.reflected_convolve_wf(_rows(dtype), k)
        assert isinstance(r, np.ndarray) and r.shape == (N_WF, LEN) and r.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_reflected_convolve_rows" and len(call) == 13
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == ["ptr", 1, 0, TAPS * esz] and call[8] == TAPS
        assert call[9] == ["ptr", 2, 0, N_WF * LEN * esz] and call[10] == LEN and call[11] is None and call[12] == "byref"
        assert fake.live() == 0
        # a 1-D call
        del fake.calls[:]
        r = processors.reflected_convolve_wf(_rows(dtype, (LEN,)), k)
        assert r.shape == (LEN,) and r.dtype == loop
        (call,) = fake.calls
        assert call[2:6] == [code, 1, LEN, LEN] and call[6] == loop_code and call[9][3] == LEN * esz and call[10] == LEN
        # a call that passes the output: written in place, returned
        del fake.calls[:]
        o = np.zeros((N_WF, LEN), dtype=loop)
        assert processors.reflected_convolve_wf(_rows(dtype), k, o) is o
        (call,) = fake.calls
        assert call[2:6] == [code, N_WF, LEN, LEN] and call[9][2:] == [0, N_WF * LEN * esz] and call[10] == LEN
        assert fake.live() == 0
        # rows, kernel and output on the device: their own memory, nothing staged
        del fake.calls[:]
        d, kd, do = DeviceArray.from_numpy(_rows(dtype)), DeviceArray.from_numpy(k.astype(loop)), DeviceArray((N_WF, LEN), loop)
        before = len(fake.device)
        assert processors.reflected_convolve_wf(d, kd, do) is do
        (call,) = fake.calls
        assert len(fake.device) == before and [call[1][1], call[7][1], call[9][1]] == [before - 3, before - 2, before - 1] and call[8] == TAPS
        d.free(), kd.free(), do.free()
        assert fake.live() == 0


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    rcw = processors.reflected_convolve_wf
    with _installed() as fake:
        with pytest.raises(NotImplementedError, match="^reflected_convolve_wf: the float64 loop takes float64 rows on the device$"):
            rcw(_rows(np.int32), np.ones(3))
        with pytest.raises(DSPFatal, match="^The filter is longer than the input waveform$"):
            rcw(_rows(np.float32), np.ones(LEN + 1))
        with pytest.raises(DSPFatal, match="^The filter is longer than the input waveform$"):
            rcw(np.full((N_WF, LEN), np.nan, np.float32), np.ones(LEN + 1))  # (for the whole call, even where every row holds a NaN)
        for rows in ("f32", "f64"):
            for n, m in rc.over_the_limit(rows):
                with pytest.raises(NotImplementedError, match=f"^reflected_convolve_wf: {rc.LIMITS} \\(len\\(w_in\\) = {n}, len\\(kernel\\) = {m} given\\): "
                                                              "a row and its mirrored margins live in 64 KiB of LDS$"):
                    rcw(np.zeros((1, n), rc.ROWS[rows]), np.ones(m))
        with pytest.raises(ValueError, match="^reflected_convolve_wf: the output has the length of the input \\(len\\(w_in\\) = 16, len\\(w_out\\) = 17\\)$"):
            rcw(_rows(np.float32), np.ones(3), np.zeros((N_WF, LEN + 1), np.float32))
        with pytest.raises(ValueError, match="the kernel holds at least one tap \\(0 given\\)"):
            rcw(_rows(np.float32), np.ones(0))
        with pytest.raises(NotImplementedError, match="per-waveform kernels are not supported"):
            rcw(_rows(np.float32), np.ones((N_WF, 3)))
        with pytest.raises(TypeError, match="takes 2 or 3 arguments"):
            rcw(_rows(np.float32))
        kd = DeviceArray.from_numpy(np.ones(3, np.float64))
        with pytest.raises(TypeError, match="a kernel on the device is one row of float32 values in the float32 loop"):
            rcw(_rows(np.float32), kd)
        kd.free()
        assert fake.calls == [] and fake.live() == 0


def test_gaussian_filter1d_is_a_host_generator():
    from dspeed_amd import processors

    with _installed() as fake:
        k = np.empty(9, np.float32)
        assert processors.gaussian_filter1d(np.float32(1), np.float32(4), k) is k and abs(float(k.sum()) - 1) < 1e-6
        assert fake.calls == [] and fake.device == []  # nothing of the library, nothing on the device


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _filter(source="waveform", module=f"{M}.convolutions", kernel="db.kernel", declared="wf_gaus"):
    return {"wf_gaus": {"function": "reflected_convolve_wf", "module": module, "args": [source, kernel, declared], "unit": "ADC"}}


def _kernel():
    from dspeed_amd.processors import gaussian_filter1d

    return gaussian_filter1d(np.float32(1), np.float32(4), np.empty(9, np.float32))


def _table(rows=None):
    from dspeed_amd.processing_chain import WaveformInput

    w = hc.sipm_rows() if rows is None else rows
    return {"waveform": WaveformInput(w, 16.0), "bl": np.full(len(w), 2000, np.float32)}


def _build(procs, outputs, table=None, db=None):
    from dspeed_amd.processing_chain import build_processing_chain

    return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table(), db_dict={"kernel": _kernel()} if db is None else db)


FRAGMENT_OUT = ["fwhm", "idx_out_c", "max_out", "vt_max_candidate_out", "vt_min_out", "n_max_out", "n_min_out"]


def test_the_sipm_fragment_behind_the_filter_is_one_launch_that_writes_the_current_only():
    for module in (f"{M}.convolutions", M):  # both module strings resolve it
        procs = {**_filter(module=module), **hc.sipm_fragment("wf_gaus")}
        chain, _, out = _build(procs, FRAGMENT_OUT)
        stages = _stages(chain)
        mine = [s for s in stages if s[1] == KERNEL]
        assert mine == [("reflected_convolve_wf wf_gaus + avg_current curr in one launch on rows", KERNEL, [L, RC, AC, ST])]
        (stage,) = [st for st in chain._stages if "reflected_convolve_wf" in st["what"]]
        assert [o[0] for o in stage["outs"]] == ["out:curr"]  # curr, not wf_gaus
        assert stages.index(mine[0]) == 0 and [s[1] for s in stages].count("dsp_hist_kernel") == 1 and "dsp_extrema_kernel" in [s[1] for s in stages]
        assert not any("-> HBM" in s[0] for s in stages)  # (nothing is written first: the histogram and the peak finder read the stage's rows)
        assert out["n_max_out"].shape == (24,)
    # the filtered waveform an output: the same launch writes both
    chain, _, out = _build({**_filter(), **hc.sipm_fragment("wf_gaus")}, FRAGMENT_OUT + ["wf_gaus", "curr"])
    (mine,) = [s for s in _stages(chain) if s[1] == KERNEL]
    assert mine[2] == [L, RC, AC, ST, ST]
    (stage,) = [st for st in chain._stages if "reflected_convolve_wf" in st["what"]]
    assert sorted(o[0] for o in stage["outs"]) == ["out:curr", "out:wf_gaus"]
    assert out["wf_gaus"].shape == (24, 1000) and out["wf_gaus"].dtype == np.float32 and out["curr"].shape == (24, 995)
    # another reader of the filtered waveform: written too
    procs = {**_filter(), **hc.sipm_fragment("wf_gaus"),
             "t_min, t_max, g_min, g_max": {"function": "min_max", "module": M, "args": ["wf_gaus", "t_min", "t_max", "g_min", "g_max"]}}
    chain, _, out = _build(procs, FRAGMENT_OUT + ["g_max"])
    (mine,) = [s for s in _stages(chain) if s[1] == KERNEL]
    assert mine[2] == [L, RC, AC, ST, ST]


def test_the_filter_alone_its_sources_and_its_kernels():
    chain, _, out = _build(_filter(), ["wf_gaus"])
    assert _stages(chain) == [("reflected_convolve_wf wf_gaus on rows", KERNEL, [L, RC, ST])] and out["wf_gaus"].shape == (24, 1000)
    # a slice of the input; a waveform the program computes, written to memory first
    chain, _, out = _build(_filter("waveform[100:900]"), ["wf_gaus"])
    io = chain._stages[0]["program"].io
    assert [(i[3], i[4]) for i in io if i[1] == _lib.IO_WF_IN] == [(800, 100)] and out["wf_gaus"].shape == (24, 800)
    blsub = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]}}
    chain, _, out = _build({**blsub, **_filter("wf_blsub")}, ["wf_gaus"])
    whats = [s[0] for s in _stages(chain)]
    assert whats.index("wf_blsub -> HBM") < whats.index("reflected_convolve_wf wf_gaus on rows")
    # another database array, the output declared with its length
    chain, _, out = _build(_filter(kernel="db.other", declared="wf_gaus(len(waveform))"), ["wf_gaus"], db={"other": np.array([1, 2, 3, 2, 1], np.float32)})
    (stage,) = chain._stages
    (taps,) = [v for k, v in stage["consts"].items() if k.startswith("taps:")]
    assert np.array_equal(taps, np.array([1, 2, 3, 2, 1], np.float32))
    # an avg_current that does not qualify stays in the program: a length per event
    procs = {**_filter(), "curr": {"function": "avg_current", "module": M, "args": ["wf_gaus", 5, "curr(len(wf_gaus)-5)"]},
             "other": {"function": "avg_current", "module": M, "args": ["waveform", 5, "other(len(waveform)-5)"]}}
    chain, _, out = _build(procs, ["curr", "other"])
    (mine,) = [s for s in _stages(chain) if s[1] == KERNEL]
    assert mine[2] == [L, RC, AC, ST] and AC in [op[0] for op in chain._program.ops]  # (the one of the raw rows)


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import WaveformInput

    with pytest.raises(DSPFatal, match="The filter is longer than the input waveform"):
        _build(_filter(), ["wf_gaus"], _table(np.full((4, 8), 2000, np.uint16)))
    with pytest.raises(ValueError, match="reflected_convolve_wf \\(wf_gaus\\): the output has the length of the input \\(len\\(w_in\\) = 1000, len\\(w_out\\) = 999\\)"):
        _build(_filter(declared="wf_gaus(999)"), ["wf_gaus"])
    with pytest.raises(NotImplementedError, match=f"reflected_convolve_wf \\(wf_gaus\\): {rc.LIMITS} \\(len\\(w_in\\) = 16380, len\\(kernel\\) = 9 given\\)"):
        _build(_filter(), ["wf_gaus"], _table(np.full((2, 16380), 2000, np.uint16)))
    with pytest.raises(NotImplementedError, match="reflected_convolve_wf \\(wf_gaus\\): the kernel is one constant array for every row.*not a per-event value"):
        _build(_filter(kernel="waveform[0:9]"), ["wf_gaus"])
    with pytest.raises(Exception, match="reflected_convolve_wf"):
        _build(_filter(module=f"{M}.fft"), ["wf_gaus"])  # not its file
    with pytest.raises(NotImplementedError, match="processor 'gaussian_filter1d' is not implemented on the device path"):  # (pinned by an existing test)
        _build({"k": {"function": "gaussian_filter1d", "module": M, "args": ["1", "4", "k(9, 'f')"]}, **_filter(kernel="k")}, ["wf_gaus"])
    tb64 = {"waveform": WaveformInput(hc.sipm_rows().astype(np.float64), 16.0)}
    with pytest.raises(NotImplementedError, match="reflected_convolve_wf in a recipe whose loop type is float64"):
        _build(_filter(), ["wf_gaus"], tb64)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="reflected_convolve_wf runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        _build(_filter(), ["wf_gaus"])
