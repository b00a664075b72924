"""The planner's, the registry's and the recipe compiler's part of interpolating_upsampler without a device (dsp_chain_plan):
DSP_OP_INTERP_UPSAMPLE has one route -- dsp_interp_kernel, whatever the switches say --, one program shape and every refusal by name; the
opcode is appended; the processor is an attribute of the registry listed in ``RESAMPLING``; what a call hands to the library (against a
subclass of tests/fake_dsp_lib.FakeLib); the stage list of the reference's docstring recipe."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import fake_dsp_lib
import interp_cases as ic
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import DSPFatal, ProcessingChainError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = ic.KERNEL
F64 = dict(rows=np.float64, loop=np.float64)
NAME = "interpolating_upsampler"


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_shape_takes_the_interp_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for n, m in ic.pairs("f32"):
            for mode in ic.modes_for("f32", n, m):
                assert plan(ic.program(n, m, mode))["kernel"] == KERNEL
        for n, m in ic.pairs("f64"):
            for mode in ic.modes_for("f64", n, m):
                assert plan(ic.program(n, m, mode, **F64), np.float64)["kernel"] == KERNEL
        assert plan(ic.program(1000, 10000, "s", np.int16))["kernel"] == KERNEL
        assert plan(ic.program(1000, 1500, "h", np.uint16, offset=3, row_stride=1007, out_stride=1505))["kernel"] == KERNEL
        assert plan(ic.program(1000, 999, "n", offset=1, row_stride=1004))["kernel"] == KERNEL
        assert plan(ic.program(1000, 1, "c", offset=2, row_stride=1010, **F64), np.float64)["kernel"] == KERNEL

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_geometry_the_case_book_assumes_is_the_headers():
    """a wavefront per row, four rows to a workgroup, up to 8 KiB of LDS a row; a workgroup per row above (the launch geometry itself:
    tests/interp_index.cpp for every length, tests/test_gpu_interp.py on the device)"""
    header = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    assert "constexpr int WAVE_ROW_BYTES = 8 * 1024, LDS_MAX = 64 * 1024;" in header and "constexpr int WARM = 48, STATIONARY = 15;" in header
    assert (ic.wide("l", 2048, 4), ic.wide("l", 2049, 4), ic.wide("s", 682, 4), ic.wide("s", 683, 4)) == (False, True, False, True)
    assert (ic.wide("l", 1024, 8), ic.wide("l", 1025, 8), ic.wide("s", 512, 8), ic.wide("s", 513, 8)) == (False, True, False, True)
    assert ic.row_bytes("s", 5456, 4) <= 65536 < ic.row_bytes("s", 5457 + 15, 4) and ic.row_bytes("s", 4096, 8) == 65536


def test_the_limits_by_name():
    assert (_lib.INTERP_F32_MAX, _lib.INTERP_SPLINE_F32_MAX, _lib.INTERP_SPLINE_F64_MAX) == (16384, 5456, 4096)
    header = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_program.h")).read()
    for line in ("#define DSP_INTERP_F32_MAX 16384", "#define DSP_INTERP_SPLINE_F32_MAX 5456", "#define DSP_INTERP_SPLINE_F64_MAX 4096"):
        assert line in header
    plan(ic.program(16384, 20000, "l")), plan(ic.program(8192, 9000, "h", **F64), np.float64)
    plan(ic.program(5456, 6000, "s")), plan(ic.program(4096, 5000, "s", **F64), np.float64)
    plan(ic.program(10, 1 << 20, "l"))  # m has no limit of its own: every program's rule for a slot, 2^20 samples
    with pytest.raises(ValueError, match="slot 1: 1048577 samples"):
        plan(ic.program(10, (1 << 20) + 1, "l"))
    for n in (16385, 20000, 1 << 19):
        with pytest.raises(NotImplementedError, match=f"{NAME}: {ic.LIMITS} \\({n} given\\): a row lives in 64 KiB of LDS"):
            plan(ic.program(n, n + 1, "l"))
    for n in (8193, 16384):
        with pytest.raises(NotImplementedError, match=f"{NAME}: {ic.LIMITS} \\({n} given\\)"):
            plan(ic.program(n, 2 * n, "f", **F64), np.float64)
    with pytest.raises(NotImplementedError, match=f"{NAME}: {ic.SPLINE_LIMITS} \\(5457 given\\): the row and its second derivatives live in 64 KiB of LDS"):
        plan(ic.program(5457, 6000, "s"))
    with pytest.raises(NotImplementedError, match=f"{NAME}: {ic.SPLINE_LIMITS} \\(4097 given\\)"):
        plan(ic.program(4097, 6000, "s", **F64), np.float64)


def test_mode_and_ratio_refusals_in_the_references_words():
    for mode in ("x", "I", 0, 300, -1):
        with pytest.raises(ValueError, match="Unrecognized interpolation mode"):
            plan(ic.program(100, 200, mode))
    with pytest.raises(ValueError, match=f"{NAME} requires len\\(w_out\\) to be an integer multiple of len\\(w_in\\) for mode 'i' \\(250 and 100 given\\)"):
        plan(ic.program(100, 250, "i"))
    with pytest.raises(ValueError, match="integer multiple"):
        plan(ic.program(100, 50, "i"))
    plan(ic.program(100, 100, "i")), plan(ic.program(1, 7, "i"))
    with pytest.raises(NotImplementedError, match=f"{NAME}: mode 'h' takes rows of at least 2 samples \\(1 given\\): the reference reads an unbound variable there"):
        plan(ic.program(1, 10, "h"))
    plan(ic.program(1, 10, "s")), plan(ic.program(2, 10, "h"))  # ('s' at n == 1 leaves the NaNs: kept)


def test_any_other_program_with_the_op_is_refused_by_name():
    shape = ("DSP_OP_INTERP_UPSAMPLE \\(interpolating_upsampler\\) runs on dsp_interp_kernel only, on rows in memory: the program must be exactly "
             "LOAD, INTERP_UPSAMPLE, STORE")
    p = ic.program(100, 1000)
    p.ops.pop()  # no store
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = ic.program(100, 1000)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = ic.program(100, 1000)
    p.n_sregs = 4
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=1)  # a second reader of the resampled row
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = ic.program(100, 100)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # destination = source
    with pytest.raises(ValueError, match="bad INTERP_UPSAMPLE \\(src: the slot of the row; dst: another slot, for the resampled row; ip\\[0\\]: the mode\\)"):
        plan(p)
    with pytest.raises((NotImplementedError, ValueError)):
        plan(ic.program(100, 1000, out_len=999))  # a store that is not the slot's length
    for rows in (np.int32, np.uint32):
        with pytest.raises(NotImplementedError, match="DSP_OP_INTERP_UPSAMPLE.*the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(ic.program(100, 1000, "l", rows, np.float64), np.float64)
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(ic.program(100, 1000, "l", np.float64, np.float32))


def test_the_opcode_is_appended_and_the_registry_lists_the_processor_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _PROCESSOR_FILES, module_accepted

    assert (_lib.OP_SORT, _lib.OP_INTERP_UPSAMPLE) == (41, 42)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_INTERP_UPSAMPLE 42" in header and "#define DSP_OP_SORT 41" in header
    assert "dsp_interp_upsample_rows_f32" not in header and "dsp_interp_upsample_rows_f64" not in header  # one entry, the loop an argument
    assert processors.RESAMPLING == (NAME,)
    assert not set(processors.RESAMPLING) & (set(processors.__all__) | set(processors.SPECTRAL) | set(processors.ORDER) | set(_PROCESSOR_FILES))
    g = processors.interpolating_upsampler
    assert g.signature == "(n),(),(m)" and g.types == ["fbf", "dbd"] and (g.nin, g.nout) == (3, 0) and g.__name__ == NAME
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "dsp_interp_upsample_rows") and "dsp_interp_upsample_rows" in _lib.EXPORTS
    assert module_accepted(M, NAME) and module_accepted(f"{M}.upsampler", NAME) and module_accepted("dspeed_amd.processors", NAME)
    assert not module_accepted(f"{M}.sort", NAME) and not module_accepted(f"{M}.upsampler", "sort") and module_accepted(f"{M}.upsampler", "upsampler")


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entry that names its loop in an argument instead of a suffix"""

    def dsp_interp_upsample_rows(self, *args):
        self.calls.append(["dsp_interp_upsample_rows"] + [self._name(a) for a in args])
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


N_WF, LEN, OUT = 3, 16, 40


def _rows(dtype, shape=(N_WF, LEN)):
    return (np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)


@pytest.mark.parametrize("dtype, code, loop_code, loop", [(np.float32, _lib.F32, _lib.F32, np.float32), (np.int16, _lib.I16, _lib.F32, np.float32),
                                                          (np.uint16, _lib.U16, _lib.F32, np.float32), (np.float64, _lib.F64, _lib.F64, np.float64)])
def test_the_arguments_of_a_call(dtype, code, loop_code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, the mode, the output, its length and stride, the stream, the row of an error"""
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    up = processors.interpolating_upsampler
    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    with _installed() as fake:
        o = np.zeros((N_WF, OUT), dtype=loop)
        assert up(_rows(dtype), "s", o) is o  # written in place, returned
        (call,) = fake.calls
        assert call[0] == "dsp_interp_upsample_rows" and len(call) == 13
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code and call[7] == ord("s")
        assert call[8] == ["ptr", 1, 0, N_WF * OUT * esz] and call[9:11] == [OUT, OUT] and call[11] is None and call[12] == "byref"
        assert fake.live() == 0
        # a 1-D call, the mode as a code
        del fake.calls[:]
        o1 = np.zeros(OUT, dtype=loop)
        assert up(_rows(dtype, (LEN,)), np.int8(ord("h")), o1) is o1
        (call,) = fake.calls
        assert call[2:6] == [code, 1, LEN, LEN] and call[7] == ord("h") and call[8][3] == OUT * esz and call[9:11] == [OUT, OUT]
        # rows and output on the device: their own memory, nothing staged
        del fake.calls[:]
        d, do = DeviceArray.from_numpy(_rows(dtype)), DeviceArray((N_WF, OUT), loop)
        before = len(fake.device)
        assert up(d, "l", do) is do
        (call,) = fake.calls
        assert len(fake.device) == before and call[1][1] == before - 2 and call[8][1] == before - 1 and call[2:6] == [code, N_WF, LEN, LEN]
        d.free(), do.free()
        assert fake.live() == 0


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors

    up = processors.interpolating_upsampler
    f32 = np.float32
    with _installed() as fake:
        with pytest.raises(TypeError, match=f"^{NAME}\\(w_in, mode_in, w_out\\): w_out must be passed \\(its length is the output size\\)$"):
            up(_rows(f32), "l")
        with pytest.raises(TypeError, match="w_out must be passed"):
            up(_rows(f32), "l", None)
        with pytest.raises(NotImplementedError, match=f"^{NAME}: the float64 loop takes float64 rows on the device$"):
            up(_rows(np.int32), "l", np.zeros((N_WF, OUT)))
        with pytest.raises(DSPFatal, match="^Unrecognized interpolation mode$"):
            up(_rows(f32), "x", np.zeros((N_WF, OUT), f32))
        with pytest.raises(DSPFatal, match=f"^{NAME} requires len\\(w_out\\) to be an integer multiple of len\\(w_in\\) for mode 'i'$"):
            up(_rows(f32), "i", np.zeros((N_WF, OUT), f32))
        with pytest.raises(NotImplementedError, match=f"^{NAME}: mode_in is a constant of the call on the device, not a per-event value$"):
            up(_rows(f32), np.array([ord("l"), ord("n"), ord("l")], np.int8), np.zeros((N_WF, OUT), f32))
        with pytest.raises(NotImplementedError, match=f"^{NAME}: mode 'h' takes rows of at least 2 samples \\(1 given\\)"):
            up(np.zeros((2, 1), f32), "h", np.zeros((2, 5), f32))
        with pytest.raises(NotImplementedError, match=f"^{NAME}: {ic.LIMITS} \\(16385 given\\): a row lives in 64 KiB of LDS$"):
            up(np.zeros((1, 16385), f32), "l", np.zeros((1, 5), f32))
        with pytest.raises(NotImplementedError, match=f"^{NAME}: {ic.LIMITS} \\(8193 given\\)"):
            up(np.zeros((2, 8193), np.float64), "c", np.zeros((2, 5), np.float64))
        with pytest.raises(NotImplementedError, match=f"^{NAME}: {ic.SPLINE_LIMITS} \\(5457 given\\)"):
            up(np.zeros((1, 5457), f32), "s", np.zeros((1, 5), f32))
        with pytest.raises(NotImplementedError, match=f"^{NAME}: {ic.SPLINE_LIMITS} \\(4097 given\\)"):
            up(np.zeros((1, 4097), np.float64), "s", np.zeros((1, 5), np.float64))
        with pytest.raises(TypeError, match="w_out is float32 in the float32 loop \\(float64 given\\)"):
            up(_rows(f32), "l", np.zeros((N_WF, OUT), np.float64))
        with pytest.raises(ValueError, match="Outputs are not the right shape"):
            up(_rows(f32), "l", np.zeros((N_WF + 1, OUT), f32))
        assert fake.calls == [] and fake.live() == 0


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _recipe(mode="'s'", source="waveform", first=None, declared=None, module=M):
    """the reference's docstring example (upsampler.py:91-102), min_max and time_point_thresh of the upsampled row behind it"""
    procs = dict(first or {})
    procs["wf_up"] = {"function": NAME, "module": module, "args": [source, mode, declared or f"wf_up(len({source})*10, period={source}.period/10)"]}
    procs["tp_min, tp_max, wf_min, wf_max"] = {"function": "min_max", "module": M, "args": ["wf_up", "tp_min", "tp_max", "wf_min", "wf_max"]}
    procs["tp_50"] = {"function": "time_point_thresh", "module": M, "args": ["wf_up", "0.5*(wf_max+wf_min)", "tp_max", 0, "tp_50"]}
    return procs


def _table(n=100, rows=12):
    from dspeed_amd.processing_chain import WaveformInput

    rng = np.random.default_rng(7)
    return {"waveform": WaveformInput((10000 + rng.integers(-20, 21, (rows, n))).astype(np.uint16), 16.0), "bl": rng.uniform(9990, 10010, rows).astype(np.float32)}


OUTPUTS = ["tp_50", "wf_max", "tp_max"]


def test_the_stage_list_of_the_docstring_recipe():
    from dspeed_amd.processing_chain import build_processing_chain

    for module in (M, f"{M}.upsampler"):
        chain, _, out = build_processing_chain({"outputs": OUTPUTS, "processors": _recipe(module=module)}, _table())
        assert _stages(chain) == [(f"{NAME} wf_up on rows", KERNEL, [_lib.OP_LOAD, _lib.OP_INTERP_UPSAMPLE, _lib.OP_STORE])]  # (a chain input: nothing written first)
        st = chain._stages[0]["program"]
        assert st.ops[1][4][0] == ord("s") and [(io[1], io[3]) for io in st.io] == [(_lib.IO_WF_IN, 100), (_lib.IO_WF_OUT, 1000)]
        assert out["tp_50"].shape == (12,)
        # the program then loads wf_up, a binding the stage wrote, and reduces it
        ops = [op[0] for op in chain._program.ops]
        assert _lib.OP_INTERP_UPSAMPLE not in ops and ops[0] == _lib.OP_LOAD and _lib.OP_MIN_MAX in ops and _lib.OP_TIME_POINT_THRESH in ops
        loads = [chain._program.io[op[3]] for op in chain._program.ops if op[0] == _lib.OP_LOAD]
        assert [(io[0], io[3]) for io in loads] == [("in:wf_up", 1000)]
    chain, _, out = build_processing_chain({"outputs": OUTPUTS + ["wf_up"], "processors": _recipe("'l'", declared="wf_up(250)")}, _table())
    assert out["wf_up"].shape == (12, 250) and out["wf_up"].dtype == np.float32


def test_sources_a_slice_and_a_waveform_the_program_computes():
    from dspeed_amd.processing_chain import build_processing_chain

    blsub = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]}}
    chain, _, out = build_processing_chain({"outputs": OUTPUTS, "processors": _recipe("'h'", "wf_blsub", blsub)}, _table())
    stages = _stages(chain)
    whats = [s[0] for s in stages]
    assert whats.index("wf_blsub -> HBM") < whats.index(f"{NAME} wf_up on rows") and [s[1] for s in stages].count(KERNEL) == 1
    chain, _, out = build_processing_chain({"outputs": OUTPUTS + ["wf_up"], "processors": _recipe("'n'", "waveform[10:90]", declared="wf_up(800)")}, _table())
    io = chain._stages[0]["program"].io
    assert [(i[3], i[4]) for i in io if i[1] == _lib.IO_WF_IN] == [(80, 10)] and not any("-> HBM" in s[0] for s in _stages(chain))
    assert out["wf_up"].shape == (12, 800)


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import build_processing_chain

    def build(procs, table=None, outputs=("wf_up",)):
        return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table())

    def one(args, module=M):
        return {"wf_up": {"function": NAME, "module": module, "args": args}}

    build(one(["waveform", "'c'", "wf_up(150)"]))
    with pytest.raises(ProcessingChainError, match=f"{NAME} \\(wf_up\\): declare the output with its length"):
        build(one(["waveform", "'l'", "wf_up"]))
    with pytest.raises(DSPFatal, match="Unrecognized interpolation mode"):
        build(one(["waveform", "'q'", "wf_up(200)"]))
    with pytest.raises(DSPFatal, match="integer multiple of len\\(w_in\\) for mode 'i'"):
        build(one(["waveform", "'i'", "wf_up(250)"]))
    with pytest.raises(NotImplementedError, match=f"{NAME} \\(wf_up\\): {ic.LIMITS} \\(16385 given\\)"):
        build(one(["waveform", "'l'", "wf_up(100)"]), _table(16385, 2))
    with pytest.raises(NotImplementedError, match=f"{NAME} \\(wf_up\\): {ic.SPLINE_LIMITS} \\(5457 given\\)"):
        build(one(["waveform", "'s'", "wf_up(100)"]), _table(5457, 2))
    with pytest.raises(NotImplementedError, match=f"{NAME} \\(wf_up\\): mode 'h' takes rows of at least 2 samples"):
        build(one(["waveform[5:6]", "'h'", "wf_up(10)"]))
    with pytest.raises(Exception, match=NAME):
        build(one(["waveform", "'l'", "wf_up(200)"], f"{M}.sort"))  # not the processor's file
    tb = _table()
    tb["which"] = np.full(12, ord("l"), np.int8)
    with pytest.raises(NotImplementedError, match=f"{NAME} \\(wf_up\\): the interpolation mode is a constant of the kernel, not a per-event value"):
        build(one(["waveform", "which", "wf_up(200)"]), tb)
    tb64 = {"waveform": _table()["waveform"].values.astype(np.float64)}
    with pytest.raises(NotImplementedError, match=f"{NAME} in a recipe whose loop type is float64"):
        build(one(["waveform", "'l'", "wf_up(200)"]), tb64)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match=f"{NAME} runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        build(one(["waveform", "'l'", "wf_up(200)"]))
