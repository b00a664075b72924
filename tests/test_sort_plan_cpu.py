"""The planner's, the registry's and the recipe compiler's part of sort without a device (dsp_chain_plan): DSP_OP_SORT has one route --
dsp_sort_kernel, whatever the switches say --, one program shape and every refusal by name; the opcode is appended; the processor is an
attribute of the registry listed in ``ORDER``; what a call hands to the library (against a subclass of tests/fake_dsp_lib.FakeLib); the
stage list of a recipe that reads the median off the sorted row."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import fake_dsp_lib
import sort_cases as sc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import ProcessingChainError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = sc.KERNEL
F64 = dict(rows=np.float64, loop=np.float64)


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_shape_takes_the_sort_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for n in sc.LENGTHS:
            assert plan(sc.program(n))["kernel"] == KERNEL
            if n <= sc.limit("f64"):
                assert plan(sc.program(n, **F64), np.float64)["kernel"] == KERNEL
        assert plan(sc.program(1000, np.int16))["kernel"] == KERNEL
        assert plan(sc.program(1000, np.uint16))["kernel"] == KERNEL
        assert plan(sc.program(1000, np.uint16, offset=3, row_stride=1007, out_stride=1005))["kernel"] == KERNEL
        assert plan(sc.program(1000, offset=1, row_stride=1004))["kernel"] == KERNEL
        assert plan(sc.program(1000, offset=2, row_stride=1010, **F64), np.float64)["kernel"] == KERNEL

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_limits_by_name():
    assert _lib.SORT_F32_MAX == sc.F32_MAX == 16384
    header = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_program.h")).read()
    assert "#define DSP_SORT_F32_MAX 16384" in header
    plan(sc.program(16384)), plan(sc.program(8192, **F64), np.float64)
    for n in (16385, 20000, 1 << 19):
        with pytest.raises(NotImplementedError, match=f"sort: {sc.LIMITS} \\({n} given\\): a row's keys live in 64 KiB of LDS"):
            plan(sc.program(n))
    for n in (8193, 16384):
        with pytest.raises(NotImplementedError, match=f"sort: {sc.LIMITS} \\({n} given\\)"):
            plan(sc.program(n, **F64), np.float64)


def test_any_other_program_with_the_op_is_refused_by_name():
    shape = "DSP_OP_SORT \\(sort\\) runs on dsp_sort_kernel only, on rows in memory: the program must be exactly LOAD, SORT, STORE"
    p = sc.program(1000)
    p.ops.pop()  # no store
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = sc.program(1000)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = sc.program(1000)
    p.n_sregs = 4
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=1)  # a second reader of the sorted row
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    p = sc.program(1000)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # destination = source
    with pytest.raises(ValueError, match="bad SORT \\(src: the slot of the row; dst: another slot, for the sorted row\\)"):
        plan(p)
    for out_len in (999, 1001, 1):  # an output whose length is not the input's: an argument error
        with pytest.raises(ValueError, match=f"SORT: the sorted row has the row's length \\(1000; {out_len} given\\)"):
            plan(sc.program(1000, out_len=out_len))
    for rows in (np.int32, np.uint32):
        with pytest.raises(NotImplementedError, match="DSP_OP_SORT.*the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(sc.program(1000, rows, np.float64), np.float64)
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(sc.program(1000, np.float64, np.float32))
    with pytest.raises((NotImplementedError, ValueError)):
        plan(sc.program(1000, loop=np.float64))  # float32 loop, float64 output


def test_the_opcode_is_appended_and_the_registry_lists_sort_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _PROCESSOR_FILES, module_accepted

    assert (_lib.OP_FFT, _lib.OP_SORT) == (40, 41)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_SORT 41" in header and "#define DSP_OP_FFT 40" in header
    assert processors.ORDER == ("sort",)
    assert not set(processors.ORDER) & (set(processors.__all__) | set(processors.SPECTRAL) | set(_PROCESSOR_FILES))
    g = processors.sort
    assert g.signature == "(n)->(n)" and g.types == ["f->f", "d->d"] and (g.nin, g.nout) == (1, 1) and g.__name__ == "sort"
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "dsp_sort_rows") and "dsp_sort_rows" in _lib.EXPORTS
    assert module_accepted(M, "sort") and module_accepted(f"{M}.sort", "sort") and module_accepted("dspeed_amd.processors", "sort")
    assert not module_accepted(f"{M}.fft", "sort") and not module_accepted(f"{M}.sort", "psd") and not module_accepted(f"{M}.sort", "histogram")


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entry that names its loop in an argument instead of a suffix"""

    def dsp_sort_rows(self, *args):
        self.calls.append(["dsp_sort_rows"] + [self._name(a) for a in args])
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


N_WF, LEN = 3, 16


def _rows(dtype, shape=(N_WF, LEN)):
    return (np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)


@pytest.mark.parametrize("dtype, code, loop_code, loop", [(np.float32, _lib.F32, _lib.F32, np.float32), (np.int16, _lib.I16, _lib.F32, np.float32),
                                                          (np.uint16, _lib.U16, _lib.F32, np.float32), (np.float64, _lib.F64, _lib.F64, np.float64)])
def test_the_arguments_of_a_call(dtype, code, loop_code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, the output and its stride, the stream, the row of an error"""
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    with _installed() as fake:
        # a 2-D call, the output left out: a new array of the loop's type
        r = processors.sort(_rows(dtype))
        assert isinstance(r, np.ndarray) and r.shape == (N_WF, LEN) and r.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_sort_rows" and len(call) == 11
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == ["ptr", 1, 0, N_WF * LEN * esz] and call[8] == LEN and call[9] is None and call[10] == "byref"
        assert fake.live() == 0
        # a 1-D call
        del fake.calls[:]
        r = processors.sort(_rows(dtype, (LEN,)))
        assert r.shape == (LEN,) and r.dtype == loop
        (call,) = fake.calls
        assert call[2:6] == [code, 1, LEN, LEN] and call[6] == loop_code and call[7][3] == LEN * esz and call[8] == LEN
        # a call that passes the output: written in place, returned
        del fake.calls[:]
        o = np.zeros((N_WF, LEN), dtype=loop)
        assert processors.sort(_rows(dtype), o) is o
        (call,) = fake.calls
        assert call[2:6] == [code, N_WF, LEN, LEN] and call[7][2:] == [0, N_WF * LEN * esz] and call[8] == LEN
        assert fake.live() == 0
        # rows and output on the device: their own memory, nothing staged
        del fake.calls[:]
        d, do = DeviceArray.from_numpy(_rows(dtype)), DeviceArray((N_WF, LEN), loop)
        before = len(fake.device)
        assert processors.sort(d, do) is do
        (call,) = fake.calls
        assert len(fake.device) == before and call[1][1] == before - 2 and call[7][1] == before - 1 and call[2:6] == [code, N_WF, LEN, LEN]
        d.free(), do.free()
        assert fake.live() == 0


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors

    with _installed() as fake:
        with pytest.raises(NotImplementedError, match="^sort: the float64 loop takes float64 rows on the device$"):
            processors.sort(_rows(np.int32))
        with pytest.raises(NotImplementedError, match=f"^sort: {sc.LIMITS} \\(16385 given\\): a row's keys live in 64 KiB of LDS$"):
            processors.sort(np.zeros((1, 16385), np.float32))
        with pytest.raises(NotImplementedError, match=f"^sort: {sc.LIMITS} \\(8193 given\\)"):
            processors.sort(np.zeros((2, 8193), np.float64))
        with pytest.raises(TypeError, match="takes 1 inputs and 1 outputs"):
            processors.sort(_rows(np.float32), None, None)
        with pytest.raises(ValueError, match="Outputs are not the right shape"):
            processors.sort(_rows(np.float32), np.zeros((N_WF, LEN + 1), np.float32))
        assert fake.calls == [] and fake.live() == 0


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _recipe(source="waveform", first=None, declared="wf_sorted"):
    procs = dict(first or {})
    procs["wf_sorted"] = {"function": "sort", "module": M, "args": [source, declared]}
    procs["med"] = {"function": "fixed_time_pickoff", "module": M, "args": ["wf_sorted", "len(wf_sorted)/2", "'i'", "med"]}
    return procs


def _table(n=1000, rows=12):
    from dspeed_amd.processing_chain import WaveformInput

    rng = np.random.default_rng(7)
    return {"waveform": WaveformInput((10000 + rng.integers(-20, 21, (rows, n))).astype(np.uint16), 16.0), "bl": rng.uniform(9990, 10010, rows).astype(np.float32)}


def test_the_stage_list_of_a_median():
    from dspeed_amd.processing_chain import build_processing_chain

    for declared in ("wf_sorted", "wf_sorted(len(waveform))", "wf_sorted(1000, 'float32')"):  # declared or not, as in the reference's example
        chain, _, out = build_processing_chain({"outputs": ["med"], "processors": _recipe(declared=declared)}, _table())
        assert _stages(chain) == [("sort wf_sorted on rows", KERNEL, [_lib.OP_LOAD, _lib.OP_SORT, _lib.OP_STORE])]  # (a chain input: nothing written first)
        assert out["med"].shape == (12,)
        # the program then loads wf_sorted, a binding the stage wrote, and picks the median off it
        ops = [op[0] for op in chain._program.ops]
        assert _lib.OP_SORT not in ops and ops[0] == _lib.OP_LOAD and _lib.OP_PICKOFF in ops
        loads = [chain._program.io[op[3]] for op in chain._program.ops if op[0] == _lib.OP_LOAD]
        assert [(io[0], io[3]) for io in loads] == [("in:wf_sorted", 1000)]
    chain, _, out = build_processing_chain({"outputs": ["med", "wf_sorted"], "processors": _recipe()}, _table())
    assert out["wf_sorted"].shape == (12, 1000) and out["wf_sorted"].dtype == np.float32


def test_sources_a_slice_and_a_waveform_the_program_computes():
    from dspeed_amd.processing_chain import build_processing_chain

    blsub = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]}}
    chain, _, out = build_processing_chain({"outputs": ["med"], "processors": _recipe("wf_blsub", blsub)}, _table())
    stages = _stages(chain)
    whats = [s[0] for s in stages]
    assert whats.index("wf_blsub -> HBM") < whats.index("sort wf_sorted on rows") and [s[1] for s in stages].count(KERNEL) == 1
    chain, _, out = build_processing_chain({"outputs": ["med", "wf_sorted"], "processors": _recipe("waveform[96:896]")}, _table())
    io = chain._stages[0]["program"].io
    assert [(i[3], i[4]) for i in io if i[1] == _lib.IO_WF_IN] == [(800, 96)] and not any("-> HBM" in s[0] for s in _stages(chain))
    assert out["wf_sorted"].shape == (12, 800)
    chain, _, out = build_processing_chain({"outputs": ["wf_sorted"], "processors": _recipe("wf_blsub[:500]", blsub)}, _table())
    mine = next(s for s in _stages(chain) if s[1] == KERNEL)
    assert mine[2] == [_lib.OP_LOAD, _lib.OP_SORT, _lib.OP_STORE] and out["wf_sorted"].shape == (12, 500)


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import build_processing_chain

    def build(procs, table=None, outputs=("wf_sorted",)):
        return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table())

    def one(args, module=M):
        return {"wf_sorted": {"function": "sort", "module": module, "args": args}}

    build(one(["waveform", "wf_sorted"], f"{M}.sort"))
    with pytest.raises(ProcessingChainError, match="sort \\(wf_sorted\\): 'wf_sorted' holds 999 samples, the source 1000"):
        build(one(["waveform", "wf_sorted(999)"]))
    with pytest.raises(NotImplementedError, match=f"sort \\(wf_sorted\\): {sc.LIMITS} \\(16385 given\\)"):
        build(one(["waveform", "wf_sorted"]), _table(16385, 2))
    with pytest.raises(Exception, match="sort"):
        build(one(["waveform", "wf_sorted"], f"{M}.fft"))  # not sort's file
    tb64 = {"waveform": _table()["waveform"].values.astype(np.float64)}
    with pytest.raises(NotImplementedError, match="sort in a recipe whose loop type is float64"):
        build(one(["waveform", "wf_sorted"]), tb64)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="sort runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        build(one(["waveform", "wf_sorted"]))
