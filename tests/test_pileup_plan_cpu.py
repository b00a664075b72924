"""The planner's, the registry's and the recipe compiler's part of the pile-up finder without a device (dsp_chain_plan): DSP_OP_RC_CR2 and
DSP_OP_BI_LEVEL_ZERO_CROSSING have one route -- dsp_pileup_kernel, whatever the switches say --, three program shapes (each with or without a
BL_SUBTRACT behind the LOAD) and every refusal by name; the opcodes are appended; the two processors are attributes of the registry listed
in ``PILEUP``; what a call hands to the library (against a subclass of tests/fake_dsp_lib.FakeLib); the stages of the recipe
bl_subtract -> rc_cr2 -> bi_level_zero_crossing_time_points."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import fake_dsp_lib
import pileup_cases as pc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import DSPFatal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = pc.KERNEL
F64 = dict(rows=np.float64, loop=np.float64)
L, BL, RC, BI, ST, SS = _lib.OP_LOAD, _lib.OP_BL_SUBTRACT, _lib.OP_RC_CR2, _lib.OP_BI_LEVEL_ZERO_CROSSING, _lib.OP_STORE, _lib.OP_STORE_SCALAR
SHAPES = ("DSP_OP_RC_CR2 / DSP_OP_BI_LEVEL_ZERO_CROSSING \\(rc_cr2, bi_level_zero_crossing_time_points\\) run on dsp_pileup_kernel only, on rows in memory: "
          "the program must be exactly LOAD, RC_CR2, STORE; or LOAD, BI_LEVEL_ZERO_CROSSING, STORE, STORE, STORE_SCALAR; or LOAD, RC_CR2, "
          "BI_LEVEL_ZERO_CROSSING, \\[STORE of the filtered row,\\] STORE, STORE, STORE_SCALAR")


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_shapes_take_the_pileup_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for n in pc.LENGTHS + (8192,):
            for kw in (dict(), dict(walk=True), dict(walk=True, store_row=False), dict(filter=False, walk=True)):
                assert [op[0] for op in pc.program(n, **kw).ops][1] in (RC, BI)
                assert plan(pc.program(n, **kw))["kernel"] == KERNEL
                assert plan(pc.program(n, **kw, **F64), np.float64)["kernel"] == KERNEL
                assert plan(pc.program(n, subtract="column", **kw))["kernel"] == KERNEL and plan(pc.program(n, subtract=1000.0, **kw))["kernel"] == KERNEL
        for rows in (np.int16, np.uint16):
            assert plan(pc.program(1000, rows, walk=True))["kernel"] == KERNEL
            assert plan(pc.program(1000, rows, offset=3, row_stride=1007, out_stride=1005, walk=True, list_stride=33, m=30))["kernel"] == KERNEL
        assert plan(pc.program(1000, walk=True, columns=(0, 1, 2, 3)))["kernel"] == KERNEL and plan(pc.program(1000, filter=False, walk=True, columns=(1, 3)))["kernel"] == KERNEL
        for m in (1, 5, 30, 1000, 5000):  # (the lists may be longer than the row)
            assert plan(pc.program(1000, filter=False, walk=True, m=m))["kernel"] == KERNEL
        assert plan(pc.program(1000, tau=float("nan")))["kernel"] == KERNEL  # a NaN t_tau: NaN rows, no error
        assert plan(pc.program(1000, filter=False, walk=True, operands=(float("nan"), float("inf"), -3.5, float("nan"))))["kernel"] == KERNEL
        assert [op[0] for op in pc.program(64, walk=True, subtract=1.0).ops] == [L, BL, RC, BI, ST, ST, ST, SS]

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_geometry_the_case_book_assumes_is_the_headers():
    kernels_h = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    mine = kernels_h[kernels_h.index("namespace dsp_pileup {"):kernels_h.index("}  // namespace dsp_pileup")]
    assert "constexpr int ROWS = 64, TS = 64, PITCH = TS + 1;" in mine and "MIN_FILTER_LEN = 4" in mine
    assert {63, 64, 65, 127, 128, 129} <= set(pc.LENGTHS) and {63, 64, 65, 130} <= set(pc.ROW_COUNTS) and min(pc.LENGTHS) == 4


def test_any_other_program_with_the_ops_is_refused_by_name():
    p = pc.program(1000)
    p.ops.pop()  # the filter, nothing stored
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000)
    p.ops.insert(1, (_lib.OP_POLE_ZERO, 0, 0, 0, (), (Scalar.const(100.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000)
    p.n_sregs = 4
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=1)  # a second reader of the filtered row
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000, walk=True)
    p.ops.insert(2, p.ops[1])  # two filters
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000, walk=True)
    p.ops.pop()  # the count not stored
    with pytest.raises(NotImplementedError, match="DSP_OP_RC_CR2 / DSP_OP_BI_LEVEL_ZERO_CROSSING.*the program must be exactly"):
        plan(p)
    p = pc.program(1000, walk=True)
    p.add_op(ST, src=1, io=p.add_io("out2", _lib.IO_WF_OUT, np.float32, 1000, 0, None))  # a store behind the count
    with pytest.raises(NotImplementedError, match="DSP_OP_RC_CR2 / DSP_OP_BI_LEVEL_ZERO_CROSSING.*the program must be exactly"):
        plan(p)
    p = pc.program(1000, walk=True)
    p.ops[2] = p.ops[2][:2] + (0,) + p.ops[2][3:]  # the walk of the raw row beside a filter
    with pytest.raises(NotImplementedError, match="DSP_OP_RC_CR2 / DSP_OP_BI_LEVEL_ZERO_CROSSING.*the walk in the same program reads exactly the filtered row"):
        plan(p)
    p = pc.program(1000, walk=True)
    p.ops[4] = p.ops[5]  # a list stored twice, the other never
    with pytest.raises(NotImplementedError, match="DSP_OP_RC_CR2.*the filtered row and the two lists are stored once each, whole, in the loop's type; the count once, into a DSP_U32 column"):
        plan(p)
    p = pc.program(1000, filter=False, walk=True)
    p.io[-1] = p.io[-1][:2] + (_lib.F32,) + p.io[-1][3:]  # the count into a float column
    with pytest.raises(NotImplementedError, match="DSP_OP_RC_CR2.*the count once, into a DSP_U32 column"):
        plan(p)
    p = pc.program(1000, subtract=1.0)
    p.ops[1] = p.ops[1][:4] + ((1,),) + p.ops[1][5:]  # numpy.subtract keeps NaN samples single: not the subtraction that is folded in
    with pytest.raises(NotImplementedError, match="DSP_OP_RC_CR2.*the BL_SUBTRACT behind the LOAD works on the rows in place \\(bl_subtract, ip\\[0\\] = 0\\)"):
        plan(p)
    for rows in (np.int32, np.uint32):
        with pytest.raises(NotImplementedError, match="DSP_OP_RC_CR2.*the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(pc.program(1000, rows, np.float64), np.float64)
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(pc.program(1000, np.float64, np.float32))


def test_the_planners_argument_errors():
    for n in (1, 2, 3):
        for kw in ({}, F64):
            with pytest.raises(DSPFatal, match="^The length of the waveform must be larger than 3 for the filter to work safely"):
                plan(pc.program(n, **kw), kw.get("loop", np.float32))
    assert plan(pc.program(4))["kernel"] == KERNEL and plan(pc.program(1, filter=False, walk=True))["kernel"] == KERNEL
    with pytest.raises(NotImplementedError, match="rc_cr2: t_tau is a constant of the program, not a per-event value: its coefficients are formed on the host"):
        plan(pc.program(1000, tau="column"))
    for out_len in (999, 1001, 4):
        with pytest.raises(ValueError, match=f"rc_cr2: the output has the length of the input \\(len\\(w_in\\) = 1000, len\\(w_out\\) = {out_len}\\)"):
            plan(pc.program(1000, out_len=out_len))
    with pytest.raises(ValueError, match="bi_level_zero_crossing_time_points: the output arrays are of different lengths \\(5 and 6\\)"):
        plan(pc.program(1000, filter=False, walk=True, list_lens=(5, 6)))
    for gate in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="bi_level_zero_crossing_time_points: gate_time_in is a finite number of samples"):
            plan(pc.program(1000, filter=False, walk=True, operands=(1, -1, gate, 0)))
    for t in (1.5, -0.25):
        with pytest.raises(DSPFatal, match="^The starting index must be an integer"):
            plan(pc.program(1000, walk=True, operands=(1, -1, 10, t)))
    for t in (-1, 1000, 1e9):
        with pytest.raises(DSPFatal, match="^The starting index is out of range"):
            plan(pc.program(1000, filter=False, walk=True, operands=(1, -1, 10, t)))
    assert plan(pc.program(1000, filter=False, walk=True, operands=(1, -1, 10, 999)))["kernel"] == KERNEL
    p = pc.program(1000)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # destination = source
    with pytest.raises(ValueError, match="bad RC_CR2 \\(src: the slot of the row; dst: another slot, for the filtered row; sp\\[0\\]: t_tau\\)"):
        plan(p)
    p = pc.program(1000, filter=False, walk=True)
    p.ops[1] = p.ops[1][:4] + ((1, 0),) + p.ops[1][5:]  # both lists in one slot
    with pytest.raises(ValueError, match="bad BI_LEVEL_ZERO_CROSSING \\(dst, ip\\[0\\]: the slots of polarity_out and t_trig_times_out; ip\\[1\\]: the register of the count\\)"):
        plan(p)
    source = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_plan.cpp")).read()  # (a slot holds at most 2^20 samples: the walk's own bound stands behind that one)
    assert "bi_level_zero_crossing_time_points: the float32 loop takes rows of at most 2^24 samples" in source
    assert _lib.fatal_message(35) == "RC-CR^2 filter produced nans in output."


def test_the_opcodes_are_appended_and_the_registry_lists_the_processors_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _PILEUP_FILES, _PROCESSOR_FILES, _SIGS, module_accepted

    assert (_lib.OP_REFLECTED_CONVOLVE, _lib.OP_RC_CR2, _lib.OP_BI_LEVEL_ZERO_CROSSING) == (45, 46, 47)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_RC_CR2 46" in header and "#define DSP_OP_BI_LEVEL_ZERO_CROSSING 47" in header and "#define DSP_E_RC_CR2_NAN 35" in header
    assert "dsp_rc_cr2_f32" not in header and "dsp_bi_level_zero_crossing_f32" not in header  # (one entry each, the loop an argument)
    assert processors.PILEUP == ("rc_cr2", "bi_level_zero_crossing_time_points")
    others = (set(processors.__all__) | set(processors.SPECTRAL) | set(processors.ORDER) | set(processors.RESAMPLING) | set(processors.ML)
              | set(processors.SMOOTHING) | set(_PROCESSOR_FILES))
    assert not set(processors.PILEUP) & others
    g = processors.rc_cr2
    assert g.signature == "(n),()->(n)" and g.types == ["ff->f", "dd->d"] and g.nargs == 3 and g.__name__ == "rc_cr2"
    g = processors.bi_level_zero_crossing_time_points
    assert g.signature == "(n),(),(),(),(),(),(m),(m)" and g.types == ["fffffIff", "dddddIdd"] and g.nargs == 8
    assert _SIGS["rc_cr2"] == "wsW" and _SIGS["bi_level_zero_crossing_time_points"] == "wssssSWW"
    assert _PILEUP_FILES == {"rc_cr2": ("rc_cr2",), "bi_level_zero_crossing_time_points": ("time_point_thresh",)}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for entry in ("dsp_rc_cr2_rows", "dsp_bi_level_zero_crossing_rows"):
        assert hasattr(lib, entry) and entry in _lib.EXPORTS
    assert module_accepted(M, "rc_cr2") and module_accepted(f"{M}.rc_cr2", "rc_cr2") and not module_accepted(f"{M}.time_point_thresh", "rc_cr2")
    fn = "bi_level_zero_crossing_time_points"
    assert module_accepted(M, fn) and module_accepted(f"{M}.time_point_thresh", fn) and module_accepted("dspeed_amd.processors", fn) and not module_accepted(f"{M}.rc_cr2", fn)


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entries that name their loop in an argument instead of a suffix"""

    def dsp_rc_cr2_rows(self, *args):
        self.calls.append(["dsp_rc_cr2_rows"] + [self._name(a) for a in args])
        return 0

    def dsp_bi_level_zero_crossing_rows(self, *args):
        self.calls.append(["dsp_bi_level_zero_crossing_rows"] + [self._name(a) for a in args])
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


N_WF, LEN, LISTS = 3, 16, 5


def _rows(dtype, shape=(N_WF, LEN)):
    return (np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)


CALLS = [(np.float32, _lib.F32, _lib.F32, np.float32), (np.int16, _lib.I16, _lib.F32, np.float32), (np.uint16, _lib.U16, _lib.F32, np.float32),
         (np.float64, _lib.F64, _lib.F64, np.float64)]


@pytest.mark.parametrize("dtype, code, loop_code, loop", CALLS)
def test_the_arguments_of_an_rc_cr2_call(dtype, code, loop_code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, t_tau, the output and its stride, the stream, the row of an error"""
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    with _installed() as fake:
        r = processors.rc_cr2(_rows(dtype), 18.75)  # the output left out: a new array of the loop's type
        assert isinstance(r, np.ndarray) and r.shape == (N_WF, LEN) and r.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_rc_cr2_rows" and len(call) == 12
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code and call[7] == 18.75
        assert call[8] == ["ptr", 1, 0, N_WF * LEN * esz] and call[9] == LEN and call[10] is None and call[11] == "byref"
        assert fake.live() == 0
        del fake.calls[:]
        r = processors.rc_cr2(_rows(dtype, (LEN,)), np.float32(20))  # a 1-D call
        assert r.shape == (LEN,) and r.dtype == loop
        (call,) = fake.calls
        assert call[2:6] == [code, 1, LEN, LEN] and call[7] == 20.0 and call[8][3] == LEN * esz
        del fake.calls[:]
        o = np.zeros((N_WF, LEN), dtype=loop)
        assert processors.rc_cr2(_rows(dtype), np.array([20.0]), o) is o  # the output passed: written in place, returned
        d, do = DeviceArray.from_numpy(_rows(dtype)), DeviceArray((N_WF, LEN), loop)
        before = len(fake.device)
        assert processors.rc_cr2(d, 20, do) is do  # rows and output on the device: their own memory, nothing staged
        assert len(fake.device) == before and [fake.calls[-1][1][1], fake.calls[-1][8][1]] == [before - 2, before - 1]
        d.free(), do.free()
        assert fake.live() == 0


@pytest.mark.parametrize("dtype, code, loop_code, loop", CALLS)
def test_the_arguments_of_a_walk_call(dtype, code, loop_code, loop):
    """rows, the loop's type, four operands as (column or NULL, constant), the count, the two lists, their length and stride"""
    from dspeed_amd import processors

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    walk = processors.bi_level_zero_crossing_time_points
    with _installed() as fake:
        pol, times = np.zeros((N_WF, LISTS), loop), np.zeros((N_WF, LISTS), loop)
        got = walk(_rows(dtype), 5, -5.5, np.array([4, 5, 6]), 0, None, pol, times)  # the count left out: a new uint32 array; a gate per row
        assert isinstance(got, tuple) and got[0].dtype == np.uint32 and got[0].shape == (N_WF,) and got[1] is pol and got[2] is times
        (call,) = fake.calls
        assert call[0] == "dsp_bi_level_zero_crossing_rows" and len(call) == 22
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7:11] == [None, 5.0, None, -5.5] and call[11] == ["ptr", 1, 0, N_WF * esz] and call[12] == 0.0 and call[13:15] == [None, 0.0]
        assert call[15] == ["ptr", 2, 0, N_WF * 4] and call[16] == ["ptr", 3, 0, N_WF * LISTS * esz] and call[17] == ["ptr", 4, 0, N_WF * LISTS * esz]
        assert call[18:20] == [LISTS, LISTS] and call[20] is None and call[21] == "byref"
        assert fake.live() == 0
        del fake.calls[:]
        count = np.zeros((), np.uint32)
        got = walk(_rows(dtype, (LEN,)), 5, -5, 10, 3, count, np.zeros(LISTS, loop), np.zeros(LISTS, loop))  # a 1-D call, the count passed
        assert got[0] is count and got[1].shape == (LISTS,)
        (call,) = fake.calls
        assert call[2:6] == [code, 1, LEN, LEN] and call[7:15] == [None, 5.0, None, -5.0, None, 10.0, None, 3.0] and call[18:20] == [LISTS, LISTS]


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors

    rc_cr2, walk = processors.rc_cr2, processors.bi_level_zero_crossing_time_points
    lists = np.zeros((N_WF, LISTS), np.float32), np.zeros((N_WF, LISTS), np.float32)
    with _installed() as fake:
        with pytest.raises(NotImplementedError, match="^rc_cr2: the float64 loop takes float64 rows on the device$"):
            rc_cr2(_rows(np.int32), 20)
        with pytest.raises(NotImplementedError, match="^rc_cr2: t_tau is a constant of the call on the device, not a per-event value$"):
            rc_cr2(_rows(np.float32), np.full(N_WF, 20.0))
        for n in (1, 2, 3):
            with pytest.raises(DSPFatal, match="^The length of the waveform must be larger than 3 for the filter to work safely$"):
                rc_cr2(np.zeros((2, n), np.float32), 20)
        with pytest.raises(ValueError, match="^rc_cr2: the output has the length of the input \\(len\\(w_in\\) = 16, len\\(w_out\\) = 17\\)$"):
            rc_cr2(_rows(np.float32), 20, np.zeros((N_WF, LEN + 1), np.float32))
        with pytest.raises(TypeError, match="takes 2 inputs and 1 outputs"):
            rc_cr2(_rows(np.float32))
        with pytest.raises(TypeError, match="polarity_out and t_trig_times_out must be passed"):
            walk(_rows(np.float32), 5, -5, 10, 0)
        with pytest.raises(ValueError, match="^bi_level_zero_crossing_time_points: polarity_out and t_trig_times_out share the dimension m \\(5 and 4 given\\)$"):
            walk(_rows(np.float32), 5, -5, 10, 0, None, lists[0], np.zeros((N_WF, 4), np.float32))
        with pytest.raises(ValueError, match="^bi_level_zero_crossing_time_points: polarity_out and t_trig_times_out hold at least one entry$"):
            walk(_rows(np.float32), 5, -5, 10, 0, None, np.zeros((N_WF, 0), np.float32), np.zeros((N_WF, 0), np.float32))
        for gate in (np.nan, np.inf):
            with pytest.raises(ValueError, match="^bi_level_zero_crossing_time_points: gate_time_in is a finite number of samples$"):
                walk(_rows(np.float32), 5, -5, gate, 0, None, *lists)
        with pytest.raises(NotImplementedError, match="the float64 loop takes float64 rows on the device"):
            walk(_rows(np.uint32), 5, -5, 10, 0, None, np.zeros((N_WF, LISTS)), np.zeros((N_WF, LISTS)))
        assert fake.calls == [] and fake.live() == 0


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _table(rows=None, n_rows=24, n=1000):
    from dspeed_amd.processing_chain import WaveformInput

    w = (1000 + (np.arange(n_rows * n).reshape(n_rows, n) * 7) % 41).astype(np.uint16) if rows is None else rows
    return {"waveform": WaveformInput(w, 16.0), "bl": np.full(len(w), 1000, np.float32), "thr": np.full(len(w), 5, np.float32)}


WALK = "n_crossings, polarity_out, trig_times"


def _recipe(source="wf_blsub", tau="320*ns", walk_of="wf_rc", pos=5, gate=100, lists=(20, 20), filter_module=f"{M}.rc_cr2", walk_module=f"{M}.time_point_thresh"):
    return {
        "wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]},
        "wf_rc": {"function": "rc_cr2", "module": filter_module, "args": [source, tau, "wf_rc"]},
        WALK: {"function": "bi_level_zero_crossing_time_points", "module": walk_module,
               "args": [walk_of, pos, -5, gate, 0, "n_crossings", f"polarity_out({lists[0]}, vector_len=n_crossings)", f"trig_times({lists[1]}, vector_len=n_crossings)"]},
    }


def _build(procs, outputs, table=None, db=None):
    from dspeed_amd.processing_chain import build_processing_chain

    return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table(), db_dict=db)


def test_the_pile_up_tagger_is_one_launch_with_the_subtraction_folded_in():
    for modules in ({}, dict(filter_module=M, walk_module=M)):  # both module strings resolve them
        chain, _, out = _build(_recipe(**modules), ["n_crossings", "polarity_out", "trig_times"])
        stages = _stages(chain)
        assert stages == [(f"rc_cr2 wf_rc + bi_level_zero_crossing_time_points {WALK} in one launch on rows", KERNEL, [L, BL, RC, BI, ST, ST, SS])]
        (stage,) = chain._stages
        assert [o[0] for o in stage["outs"]] == ["out:polarity_out", "out:trig_times", "out:n_crossings"]  # no filtered row, no subtracted row
        rc_op = stage["program"].ops[2]
        assert rc_op[5][0].kind == _lib.ARG_CONST and rc_op[5][0].value == 20.0  # 320 ns on a 16 ns grid
        assert stage["program"].ops[1][5][0].kind == _lib.ARG_INPUT  # the baseline: the table's column
        assert not any(op[0] in (BL, RC, BI) for op in chain._program.ops)
        assert out["n_crossings"].dtype == np.uint32 and out["n_crossings"].shape == (24,) and out["trig_times"].shape == (24, 20)
        assert chain.vector_lens == {"polarity_out": "n_crossings", "trig_times": "n_crossings"}
    # the count not asked for: a hidden output, for the lists' lengths
    chain, _, out = _build(_recipe(), ["trig_times"])
    assert chain.hidden_outputs == ["n_crossings"] and _stages(chain)[0][2] == [L, BL, RC, BI, ST, ST, SS]


def test_the_filtered_row_is_stored_when_asked_for_or_read():
    chain, _, out = _build(_recipe(), ["n_crossings", "wf_rc"])
    (mine,) = _stages(chain)
    assert mine[2] == [L, BL, RC, BI, ST, ST, ST, SS]
    assert [o[0] for o in chain._stages[0]["outs"]][0] == "out:wf_rc" and out["wf_rc"].shape == (24, 1000) and out["wf_rc"].dtype == np.float32
    # another reader of the filtered waveform: written too, and read from there
    procs = {**_recipe(), "t_min, t_max, rc_min, rc_max": {"function": "min_max", "module": M, "args": ["wf_rc", "t_min", "t_max", "rc_min", "rc_max"]}}
    chain, _, out = _build(procs, ["n_crossings", "rc_max"])
    mine = [s for s in _stages(chain) if s[1] == KERNEL]
    assert [m[2] for m in mine] == [[L, BL, RC, BI, ST, ST, ST, SS]]
    # the subtracted waveform asked for, or read by something else: written to memory first, not folded in
    chain, _, out = _build(_recipe(), ["n_crossings", "wf_blsub"])
    whats = [s[0] for s in _stages(chain)]
    assert whats.index("wf_blsub -> HBM") < whats.index(f"rc_cr2 wf_rc + bi_level_zero_crossing_time_points {WALK} in one launch on rows")
    assert [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, RC, BI, ST, ST, SS]]
    # a constant baseline is folded in as well; the filter alone
    procs = _recipe()
    procs["wf_blsub"]["args"][1] = 1000
    chain, _, out = _build(procs, ["n_crossings"])
    assert _stages(chain)[0][2] == [L, BL, RC, BI, ST, ST, SS] and chain._stages[0]["program"].ops[1][5][0].value == 1000.0
    chain, _, out = _build({k: v for k, v in _recipe().items() if k != WALK}, ["wf_rc"])
    assert _stages(chain) == [("rc_cr2 wf_rc on rows", KERNEL, [L, BL, RC, ST])]


def test_the_walk_alone_its_sources_and_its_operands():
    procs = {WALK: _recipe(walk_of="waveform")[WALK]}
    chain, _, out = _build(procs, ["n_crossings", "trig_times"])
    assert _stages(chain) == [(f"bi_level_zero_crossing_time_points {WALK} on rows", KERNEL, [L, BI, ST, ST, SS])]
    # a slice of the input; thresholds per event from the table
    procs = {WALK: _recipe(walk_of="waveform[100:900]", pos="thr")[WALK]}
    chain, _, out = _build(procs, ["n_crossings"])
    (stage,) = chain._stages
    assert [(i[3], i[4]) for i in stage["program"].io if i[1] == _lib.IO_WF_IN] == [(800, 100)]
    assert stage["program"].ops[1][5][0].kind == _lib.ARG_INPUT and stage["program"].ops[1][5][1].kind == _lib.ARG_CONST
    # the walk of a subtracted waveform without a filter: the subtraction joins its launch
    chain, _, out = _build({k: v for k, v in _recipe(walk_of="wf_blsub").items() if k != "wf_rc"}, ["n_crossings"])
    assert _stages(chain) == [(f"bi_level_zero_crossing_time_points {WALK} on rows", KERNEL, [L, BL, BI, ST, ST, SS])]
    # a filter two walks read: staged by itself, its rows read by both
    procs = _recipe()
    procs["n2, p2, t2"] = {"function": "bi_level_zero_crossing_time_points", "module": M,
                           "args": ["wf_rc", 9, -9, 50, 0, "n2", "p2(10, vector_len=n2)", "t2(10, vector_len=n2)"]}
    chain, _, out = _build(procs, ["n_crossings", "n2"])
    mine = [s[2] for s in _stages(chain) if s[1] == KERNEL]
    assert sorted(mine) == sorted([[L, BL, RC, BI, ST, ST, ST, SS], [L, BI, ST, ST, SS]])


def test_a_source_from_another_kernels_stage_is_staged_in_order():
    """a sorted row, and a smoothed one, as the source: the producer's stage first, then the pile-up kernel on its rows"""
    from dspeed_amd.processors import gaussian_filter1d

    procs = {"wf_sorted": {"function": "sort", "module": M, "args": ["waveform", "wf_sorted"]}, **_recipe(source="wf_sorted")}
    chain, _, out = _build(procs, ["n_crossings"])
    kernels = [s[1] for s in _stages(chain)]
    assert kernels.index("dsp_sort_kernel") < kernels.index(KERNEL) and [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, RC, BI, ST, ST, SS]]
    k = gaussian_filter1d(np.float32(1), np.float32(4), np.empty(9, np.float32))
    procs = {"wf_gaus": {"function": "reflected_convolve_wf", "module": M, "args": ["wf_blsub", "db.kernel", "wf_gaus"]},
             **{key: v for key, v in _recipe(walk_of="wf_gaus").items() if key != "wf_rc"}}
    chain, _, out = _build(procs, ["n_crossings", "trig_times"], db={"kernel": k})
    kernels = [s[1] for s in _stages(chain)]
    assert kernels.index("dsp_reflect_kernel") < kernels.index(KERNEL) and [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, BI, ST, ST, SS]]


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import WaveformInput

    with pytest.raises(DSPFatal, match="The length of the waveform must be larger than 3 for the filter to work safely"):
        _build(_recipe(), ["n_crossings"], _table(np.full((4, 3), 1000, np.uint16)))
    with pytest.raises(NotImplementedError, match="rc_cr2 \\(wf_rc\\): t_tau is a constant of the kernel, not a per-event value: its coefficients are formed on the host"):
        _build(_recipe(tau="thr"), ["n_crossings"])
    with pytest.raises(ValueError, match="bi_level_zero_crossing_time_points \\(n_crossings, polarity_out, trig_times\\): polarity_out and t_trig_times_out share the "
                                         "dimension m \\(20 and 19 given\\)"):
        _build(_recipe(lists=(20, 19)), ["n_crossings"])
    with pytest.raises(ValueError, match="bi_level_zero_crossing_time_points \\(.*\\): gate_time_in is a finite number of samples"):
        _build(_recipe(gate=float("inf")), ["n_crossings"])
    with pytest.raises(Exception, match="rc_cr2"):
        _build(_recipe(filter_module=f"{M}.time_point_thresh"), ["n_crossings"])  # not its file
    tb64 = {"waveform": WaveformInput(np.full((4, 100), 1000.0), 16.0), "bl": np.full(4, 1000.0)}
    with pytest.raises(NotImplementedError, match="(rc_cr2|bi_level_zero_crossing_time_points) in a recipe whose loop type is float64"):
        _build(_recipe(), ["n_crossings"], tb64)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="(rc_cr2|bi_level_zero_crossing_time_points) runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        _build(_recipe(), ["n_crossings"])


def test_build_dsp_clips_the_lists_lengths_to_what_was_declared():
    """the count goes on past the lists' length: the lists leave with the declared length at most, the count as the reference counts it"""
    import importlib

    bd = importlib.import_module("dspeed_amd.build_dsp")

    class _Chain:
        _out_vars = {"out:n": (None, None), "out:t": (None, 5)}
        _copy_pars, vector_lens, hidden_outputs, loop_dtype = (), {"t": "n"}, [], np.float32

        def __call__(self, columns, out):
            out["n"][:] = [0, 3, 5, 49]
            out["t"][:] = 7

    worker = bd._ChunkWorker.__new__(bd._ChunkWorker)
    worker.chain, worker.buffer_len, worker.mask = _Chain(), 4, None
    real = bd._set_buffer_len
    bd._set_buffer_len = lambda *a: None
    try:
        out, lens = worker.process(0, 4, {})
    finally:
        bd._set_buffer_len = real
    assert list(lens["t"]) == [0, 3, 5, 5] and list(out["n"]) == [0, 3, 5, 49]
