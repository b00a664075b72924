"""The planner's, the registry's and the recipe compiler's part of the waveform aligner without a device (dsp_chain_plan): DSP_OP_INL_CORRECTION,
DSP_OP_WF_CENTROID, DSP_OP_WF_ALIGNMENT and DSP_OP_WF_CORRECTION have one route -- dsp_align_kernel, whatever the switches say --, their five
program shapes and every refusal by name; the opcodes and error codes are appended; the five processors are attributes of the registry listed
in ``ALIGNMENT``; what a call hands to the library (against a subclass of tests/fake_dsp_lib.FakeLib); every check text; the stages of the recipe
inl_correction -> convolve_wf with step -> get_wf_centroid -> wf_alignment -> wf_correction, fused and apart."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import align_cases as ac
import fake_dsp_lib
from dspeed_amd import _lib
from dspeed_amd.chain import plan
from dspeed_amd.errors import DSPFatal, ProcessingChainError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = ac.KERNEL
L, IN, CE, AL, CO, ST, SS = (_lib.OP_LOAD, _lib.OP_INL_CORRECTION, _lib.OP_WF_CENTROID, _lib.OP_WF_ALIGNMENT, _lib.OP_WF_CORRECTION, _lib.OP_STORE, _lib.OP_STORE_SCALAR)
NAMES = ("DSP_OP_INL_CORRECTION / DSP_OP_WF_CENTROID / DSP_OP_WF_ALIGNMENT / DSP_OP_WF_CORRECTION \\(inl_correction, get_wf_centroid, wf_alignment, wf_correction\\) run on "
         "dsp_align_kernel only, on rows in memory: ")
SHAPES = NAMES + ("the program must be exactly LOAD, INL_CORRECTION, STORE; or LOAD, WF_CENTROID, STORE_SCALAR; or LOAD, WF_ALIGNMENT, STORE; or LOAD, WF_CORRECTION, STORE; "
                  "or LOAD, WF_ALIGNMENT, WF_CORRECTION, \\[STORE of the aligned row,\\] STORE")
EVERY_SHAPE = [(dict(op="inl"), [L, IN, ST]), (dict(op="centroid"), [L, CE, SS]), (dict(op="align"), [L, AL, ST]), (dict(op="correct"), [L, CO, ST]),
               (dict(op="fused"), [L, AL, CO, ST, ST]), (dict(op="fused", store_aligned=False), [L, AL, CO, ST])]


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_every_shape_takes_the_align_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for kw, ops in EVERY_SHAPE:
            assert [op[0] for op in ac.program(129, **kw).ops] == ops
            for n in ac.LENGTHS + (1 << 20,):
                size = min(10, n)
                assert plan(ac.program(n, size=size, **kw))["kernel"] == KERNEL, (kw, n)
                assert plan(ac.program(n, size=size, loop=np.float64, **kw), np.float64)["kernel"] == KERNEL
            assert plan(ac.program(1000, offset=3, row_stride=1007, out_stride=1005, **kw))["kernel"] == KERNEL
        for rows in (np.int16, np.uint16, np.int32, np.uint32):  # integer rows: inl_correction's only, in both loops; wf_alignment's too, int32 / uint32 in the float64 loop
            for loop in (np.float32, np.float64):
                for op in ("inl", "align", "fused"):
                    if op == "inl" or loop is np.float64 or rows in (np.int16, np.uint16):
                        assert plan(ac.program(1000, op, rows=rows, loop=loop), loop)["kernel"] == KERNEL
        for rows in (np.int16, np.uint16):
            for op in ("centroid", "correct"):
                assert plan(ac.program(1000, op, rows=rows))["kernel"] == KERNEL
        assert plan(ac.program(1000, "align", centroid="column"))["kernel"] == KERNEL and plan(ac.program(1000, "fused", centroid="column", loop=np.float64), np.float64)["kernel"] == KERNEL
        for p in (1, 256, 65536):
            assert plan(ac.program(1000, "inl", table_len=p))["kernel"] == KERNEL

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_any_other_program_with_the_ops_is_refused_by_name():
    from dspeed_amd.chain import Scalar

    for op in ("inl", "centroid", "align", "correct", "fused"):
        p = ac.program(1000, op)
        p.ops.pop()  # nothing stored (the fused pair: the corrected row not stored)
        with pytest.raises(NotImplementedError, match=NAMES):
            plan(p)
        p = ac.program(1000, op)
        p.ops.insert(1, (_lib.OP_POLE_ZERO, 0, 0, 0, (), (Scalar.const(100.0),)))  # an intermediate as the source
        with pytest.raises(NotImplementedError, match=SHAPES):
            plan(p)
        p = ac.program(1000, op)
        p.ops.append(p.ops[-1])  # stored twice
        with pytest.raises(NotImplementedError, match=NAMES):
            plan(p)
    p = ac.program(1000, "align")
    p.ops.insert(2, p.ops[1])  # two alignments
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = ac.program(1000, "fused")
    p.ops[1], p.ops[2] = p.ops[2], p.ops[1]  # the correction ahead of the alignment
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = ac.program(1000, "fused", size=1000)
    p.ops[2] = p.ops[2][:2] + (0,) + p.ops[2][3:]  # the correction of the raw row beside an alignment
    with pytest.raises(NotImplementedError, match=NAMES + "wf_correction in the same program reads exactly the aligned row"):
        plan(p)
    p = ac.program(1000, "fused")
    p.ops[4] = p.ops[3]  # the aligned row stored twice, the corrected row never
    with pytest.raises(NotImplementedError, match=NAMES + "each output row is stored once, whole, in the loop's type"):
        plan(p)
    p = ac.program(1000, "inl")
    p.ops.append((CE, p.add_sregs(1), 0, 0, (), (Scalar.const(0.0),)))  # two of the family's ops that are no pair
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    for rows in (np.float32,):
        with pytest.raises(NotImplementedError, match=NAMES + "inl_correction reads DSP_I16, DSP_U16, DSP_I32 or DSP_U32 rows: an ADC code is an integer"):
            plan(ac.program(1000, "inl", rows=rows))
    with pytest.raises(NotImplementedError, match=NAMES + "inl_correction reads DSP_I16"):
        plan(ac.program(1000, "inl", rows=np.float64, loop=np.float64), np.float64)
    for op in ("centroid", "correct"):
        with pytest.raises(NotImplementedError, match=NAMES + "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(ac.program(1000, op, rows=np.int32, loop=np.float64), np.float64)
        with pytest.raises(NotImplementedError, match=NAMES + "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(ac.program(1000, op, rows=np.int32))
    why = NAMES + "wf_alignment takes the loop's float rows, DSP_I16 or DSP_U16 rows in either loop, DSP_I32 or DSP_U32 rows in the float64 loop"
    with pytest.raises(NotImplementedError, match=why):
        plan(ac.program(1000, "align", rows=np.float32, loop=np.float64), np.float64)
    for rows in (np.int32, np.uint32):  # a float32 does not hold every int32: those rows select the float64 loop, as everywhere
        for op in ("align", "fused"):
            with pytest.raises(NotImplementedError, match=why):
                plan(ac.program(1000, op, rows=rows))
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(ac.program(1000, "align", rows=np.float64))
    p = ac.program(1000, "align", centroid="column")
    p.io[1] = p.io[1][:2] + (_lib.I16,) + p.io[1][3:]  # a centroid column of another type than the loop's
    with pytest.raises(NotImplementedError, match=NAMES + "centroid is a constant or a per-event column of the loop's type"):
        plan(p)


CHECKS = [  # (what program takes, the text) -- the reference's DSPFatal texts in the reference's order
    (dict(op="centroid", shift=float("nan")), "shift is nan"), (dict(op="centroid", shift=-0.5), "shift must be positive"),
    (dict(op="centroid", shift=128.5), "shift must be shorter than input waveform size"),
    (dict(op="align", shift=float("nan"), size_arg=float("nan")), "shift is nan"), (dict(op="align", shift=-1.0, size_arg=-1.0), "shift must be positive"),
    (dict(op="align", shift=129.5), "shift must be shorter than input waveform size"), (dict(op="align", size_arg=float("nan")), "size is nan"),
    (dict(op="align", size_arg=0.0), "size must be positive"), (dict(op="align", size_arg=-3.0), "size must be positive"),
    (dict(op="align", size_arg=130.0, out_len=129), "size must be shorter than input waveform size"),
    (dict(op="align", size_arg=9.5), "wf_alignment: size is a whole number and equals len\\(w_out\\) \\(size = 9.5, len\\(w_out\\) = 10\\)"),
    (dict(op="align", size_arg=9.0), "wf_alignment: size is a whole number and equals len\\(w_out\\) \\(size = 9, len\\(w_out\\) = 10\\)"),
] + [(dict(op="correct", table_len=m, start=a, stop=b), text) for n, m, a, b, text in ac.CORRECTION_REFUSALS] + [
    (dict(op="fused", size=10, table_len=10, start=0, stop=11), "stop_idx must be shorter than input waveform size"),  # (the window is the input of the pair's correction)
]


@pytest.mark.parametrize("kw, text", CHECKS)
def test_the_planners_check_texts(kw, text):
    for loop in (np.float32, np.float64):
        with pytest.raises(ValueError, match="chain: " + text + "$"):
            plan(ac.program(129, loop=loop, **kw), loop)


def test_the_planners_argument_errors():
    from dspeed_amd.chain import Scalar

    assert plan(ac.program(129, "centroid", shift=128.0))["kernel"] == KERNEL and plan(ac.program(129, "align", shift=129.0))["kernel"] == KERNEL
    assert plan(ac.program(129, "align", size=129))["kernel"] == KERNEL and plan(ac.program(129, "correct", table_len=40, start=50, stop=90))["kernel"] == KERNEL
    with pytest.raises(DSPFatal, match="(?m)^centroid is nan$"):
        plan(ac.program(129, "align", centroid=float("nan")))
    with pytest.raises(ValueError, match="inl_correction: the output has the length of the input \\(len\\(w_in\\) = 129, len\\(w_out\\) = 128\\)"):
        plan(ac.program(129, "inl", out_len=128))
    with pytest.raises(ValueError, match="wf_correction: the output has the length of the input \\(len\\(w_in\\) = 129, len\\(w_out\\) = 130\\)"):
        plan(ac.program(129, "correct", out_len=130))
    with pytest.raises(ValueError, match="taps the compute type"):  # (every program's rule, ahead of the op's own)
        plan(ac.program(129, "inl", table_dtype=np.float64, loop=np.float32))
    p = ac.program(129, "inl")
    p.ops[1] = p.ops[1][:3] + (2,) + p.ops[1][4:]  # the output's binding where the table's belongs
    with pytest.raises(ValueError, match="inl_correction: io is a DSP_IO_TAPS binding of the p >= 1 entries of inl in the loop's type"):
        plan(p)
    with pytest.raises(ValueError):  # float32 taps in the float64 loop: no program's
        plan(ac.program(129, "correct", table_dtype=np.float32, loop=np.float64), np.float64)
    for op, name in (("inl", "INL_CORRECTION"), ("align", "WF_ALIGNMENT"), ("correct", "WF_CORRECTION")):
        p = ac.program(129, op)
        p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # destination = source
        with pytest.raises(ValueError, match=f"bad {name} \\(src: the slot of the row; dst: another slot"):
            plan(p)
    p = ac.program(129, "centroid")
    p.n_sregs = 0
    with pytest.raises(ValueError, match="bad WF_CENTROID \\(src: the slot of the row; dst: the register of the centroid\\)"):
        plan(p)
    # a per-event value where a constant is expected: refused by name
    col = lambda p: Scalar.input(p.add_io("col", _lib.IO_SCALAR_IN, np.float32))  # noqa: E731
    p = ac.program(129, "centroid")
    p.ops[1] = p.ops[1][:5] + ((col(p),),)
    with pytest.raises(NotImplementedError, match="get_wf_centroid: shift is a constant of the program, not a per-event value"):
        plan(p)
    for k, name in ((1, "shift"), (2, "size")):
        p = ac.program(129, "align")
        sp = list(p.ops[1][5])
        sp[k] = col(p)
        p.ops[1] = p.ops[1][:5] + (tuple(sp),)
        with pytest.raises(NotImplementedError, match=f"wf_alignment: {name} is a constant of the program, not a per-event value"):
            plan(p)


def test_the_opcodes_and_error_codes_are_appended_and_the_registry_lists_the_processors_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _ALIGN_FILES, _GENERATORS, _PROCESSOR_FILES, _SIGS, module_accepted

    assert (_lib.OP_POLY_EXP_RMS, _lib.OP_INL_CORRECTION, _lib.OP_WF_CENTROID, _lib.OP_WF_ALIGNMENT, _lib.OP_WF_CORRECTION) == (53, 54, 55, 56, 57)
    assert (_lib.E_INL_RANGE, _lib.E_ALIGN_CENTROID) == (37, 38)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    for line in ("#define DSP_OP_INL_CORRECTION 54", "#define DSP_OP_WF_CENTROID 55", "#define DSP_OP_WF_ALIGNMENT 56", "#define DSP_OP_WF_CORRECTION 57",
                 "#define DSP_E_INL_RANGE 37", "#define DSP_E_ALIGN_CENTROID 38"):
        assert line in header
    kernels_h = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    assert "DSP_ROUTE_ALIGN," in kernels_h and '"dsp_align_kernel",' in kernels_h
    assert processors.ALIGNMENT == ("inl_correction", "get_wf_centroid", "wf_alignment", "wf_correction", "step")
    others = (set(processors.__all__) | set(processors.SPECTRAL) | set(processors.ORDER) | set(processors.RESAMPLING) | set(processors.ML)
              | set(processors.SMOOTHING) | set(processors.PILEUP) | set(processors.PULSES) | set(processors.TAILFIT) | set(_PROCESSOR_FILES))
    assert not set(processors.ALIGNMENT) & others
    for name, sig, types in (("inl_correction", "(n),(p)->(n)", ["if->f", "id->d"]), ("get_wf_centroid", "(n),()->()", ["ff->f", "dd->d"]),
                             ("wf_alignment", "(n),(),(),(),(m)", ["fffff", "ddddd"]), ("wf_correction", "(n),(m),(),()->(n)", ["ffii->f", "ddii->d"]),
                             ("step", "(),(n)", ["ff", "dd"])):
        g = getattr(processors, name)
        assert g.signature == sig and g.types == types and g.__name__ == name
    assert _SIGS["inl_correction"] == "waW" and _SIGS["get_wf_centroid"] == "wsS" and _SIGS["wf_alignment"] == "wsssW" and _SIGS["wf_correction"] == "waiiW"
    assert "step" in _GENERATORS and {"t0_filter", "moving_slope"} <= set(_GENERATORS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dsp_fatal_message.restype = ctypes.c_char_p
    for entry in ("dsp_inl_correction_rows", "dsp_wf_centroid_rows", "dsp_wf_alignment_rows", "dsp_wf_correction_rows"):
        assert hasattr(lib, entry) and entry in _lib.EXPORTS
    assert lib.dsp_fatal_message(38) == b"centroid is nan" and lib.dsp_fatal_message(37).startswith(b"ADC code")
    for fn, file in _ALIGN_FILES.items():
        assert module_accepted(M, fn) and module_accepted("dspeed_amd.processors", fn) and module_accepted(f"{M}.{file[0]}", fn) and not module_accepted(f"{M}.rc_cr2", fn)
    assert _ALIGN_FILES["step"] == ("kernels",) and not module_accepted(f"{M}.wf_alignment", "wf_correction")


def test_step_runs_on_the_host():
    from dspeed_amd import processors

    for T in (np.float32, np.float64):
        for n in (1, 2, 3, 4, 10, 16, 17):
            k = np.zeros(n, T)
            assert processors.step(16, k) is k and np.array_equal(k, ac.emulate_step(n, T)) and k.dtype == T
    assert list(np.flatnonzero(processors.step(0.5, np.zeros(10, np.float32)) == 1)) == [3, 4, 5, 6, 7]  # weight_pos: accepted, not used


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entries that name their loop in an argument instead of a suffix"""

    def _record(self, name, args):
        self.calls.append([name] + [self._name(a) for a in args])
        return 0

    def dsp_inl_correction_rows(self, *args):
        return self._record("dsp_inl_correction_rows", args)

    def dsp_wf_centroid_rows(self, *args):
        return self._record("dsp_wf_centroid_rows", args)

    def dsp_wf_alignment_rows(self, *args):
        return self._record("dsp_wf_alignment_rows", args)

    def dsp_wf_correction_rows(self, *args):
        return self._record("dsp_wf_correction_rows", args)


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
    return (1 + np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)


CALLS = [(np.float32, _lib.F32, _lib.F32, np.float32), (np.int16, _lib.I16, _lib.F32, np.float32), (np.uint16, _lib.U16, _lib.F32, np.float32),
         (np.float64, _lib.F64, _lib.F64, np.float64)]


@pytest.mark.parametrize("dtype, code, loop_code, loop", CALLS)
def test_the_arguments_of_the_calls(dtype, code, loop_code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, then: shift, the centroid | the centroid column or None, centroid, shift,
    size, the window, its length and stride | the template, its length, start, stop, the output and its stride; the stream, the row of an error"""
    from dspeed_amd import processors

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    with _installed() as fake:
        r = processors.get_wf_centroid(_rows(dtype), 2.5)  # the output left out: a value per row in the loop's type
        assert isinstance(r, np.ndarray) and r.shape == (N_WF,) and r.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_wf_centroid_rows" and len(call) == 11
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == 2.5 and call[8] == ["ptr", 1, 0, N_WF * esz] and call[9] is None and call[10] == "byref" and fake.live() == 0
        del fake.calls[:]
        out = np.zeros((N_WF, 4), loop)
        assert processors.wf_alignment(_rows(dtype), 7.0, 1.0, 4, out) is out  # one centroid for every row
        (call,) = fake.calls
        assert call[0] == "dsp_wf_alignment_rows" and len(call) == 16 and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        k = call[1][1]  # (allocations count on from call to call)
        assert call[7] is None and call[8:11] == [7.0, 1.0, 4.0] and call[11] == ["ptr", k + 1, 0, N_WF * 4 * esz] and call[12:14] == [4, 4]
        assert call[14] is None and call[15] == "byref" and fake.live() == 0
        del fake.calls[:]
        processors.wf_alignment(_rows(dtype), np.array([7.0, 8.0, np.nan]), 1.0, 4.0, out)  # a centroid per row: a column of the loop's type; a NaN among them is the device's to find
        (call,) = fake.calls
        k = call[1][1]
        assert call[7] == ["ptr", k + 1, 0, N_WF * esz] and call[8:11] == [0.0, 1.0, 4.0] and call[11] == ["ptr", k + 2, 0, N_WF * 4 * esz]
        del fake.calls[:]
        r = processors.wf_correction(_rows(dtype), np.arange(5.0), 2, 6)  # one template for every row, cast to the loop's type
        assert r.shape == (N_WF, LEN) and r.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_wf_correction_rows" and len(call) == 15 and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        k = call[1][1]
        assert call[7] == ["ptr", k + 1, 0, 5 * esz] and call[8:11] == [5, 2, 6] and call[11] == ["ptr", k + 2, 0, N_WF * LEN * esz] and call[12] == LEN
        assert call[13] is None and call[14] == "byref" and fake.live() == 0
        del fake.calls[:]
        c = processors.get_wf_centroid(_rows(dtype, (LEN,)), 0)  # a 1-D call: one value
        assert np.ndim(c) == 0 and fake.calls[0][2:6] == [code, 1, LEN, LEN]


@pytest.mark.parametrize("dtype, code", [(np.int16, _lib.I16), (np.uint16, _lib.U16), (np.int32, _lib.I32), (np.uint32, _lib.U32)])
@pytest.mark.parametrize("loop, loop_code", [(np.float32, _lib.F32), (np.float64, _lib.F64)])
def test_the_arguments_of_inl_correction(dtype, code, loop, loop_code):
    """the table's type selects the loop, whatever integers the rows hold: rows, the loop's type, the table and its length, the output and its stride"""
    from dspeed_amd import processors

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    with _installed() as fake:
        r = processors.inl_correction(_rows(dtype), np.zeros(256, loop))
        assert r.shape == (N_WF, LEN) and r.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_inl_correction_rows" and len(call) == 13 and call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == ["ptr", 1, 0, 256 * esz] and call[8] == 256 and call[9] == ["ptr", 2, 0, N_WF * LEN * esz] and call[10] == LEN and call[11] is None and call[12] == "byref"
        assert fake.live() == 0


def test_the_range_error_names_the_first_offending_sample_of_the_row():
    from dspeed_amd import processors

    class _Raising(_Fake):
        def dsp_inl_correction_rows(self, *args):
            args[-1]._obj.value = 1  # the error word: the code and the row
            return _lib.E_INL_RANGE

    rows = _rows(np.int16)
    rows[1, 5], rows[1, 9], rows[2, 0] = 300, -2, 999
    from dspeed_amd import device
    real, bounce = _lib._lib, device._Bounce._local.__dict__.pop("buf", None)
    _lib._lib = _Raising(real)
    try:
        with pytest.raises(DSPFatal, match="(?m)^ADC code 300 out of range for INL array of length 256$") as e:
            processors.inl_correction(rows, np.zeros(256, np.float32))
        assert e.value.wf_range == range(1, 2) and e.value.processor == "inl_correction" and _lib._lib.live() == 0
    finally:
        device._Bounce._local.__dict__.pop("buf", None)
        if bounce is not None:
            device._Bounce._local.buf = bounce
        _lib._lib = real
    assert str(processors.inl_range_error(np.array([3, -2, 300]), 256)) == "ADC code -2 out of range for INL array of length 256"


def test_integer_indices_per_row_are_grouped_by_value_like_every_integer_parameter():
    """start_idx / stop_idx are 'i' of the type strings: one value per row in host memory runs a call per value (HipGUFunc's rule for every
    integer parameter, trap_filter's rise and flat among them); on the device it is refused by name"""
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    w = _rows(np.float32)
    with _installed() as fake:
        out = processors.wf_correction(w, np.arange(8.0), np.array([2, 3, 2]), 6)
        assert out.shape == (N_WF, LEN) and sorted((call[3], call[9], call[10]) for call in fake.calls) == [(1, 3, 6), (2, 2, 6)]  # (rows, start, stop) of each call
        del fake.calls[:]
        col = DeviceArray.from_numpy(np.array([2, 3, 2], np.int32))
        with pytest.raises(NotImplementedError, match="^wf_correction: start_idx is a constant of the call on the device, not a per-event value$"):
            processors.wf_correction(w, np.arange(8.0), col, 6)
        col.free()
        assert fake.calls == [] and fake.live() == 0


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors

    w = _rows(np.float32)
    out = np.zeros((N_WF, 4), np.float32)
    with _installed() as fake:
        for dtype in (np.float32, np.float64):
            with pytest.raises(TypeError, match="^inl_correction: w_in holds int16, uint16, int32 or uint32 ADC codes \\(float(32|64) given\\): the reference has no loop for anything else$"):
                processors.inl_correction(_rows(dtype), np.zeros(8, np.float32))
        with pytest.raises(NotImplementedError, match="^inl_correction: inl is one constant array of the call on the device, not an array per event$"):
            processors.inl_correction(_rows(np.uint16), np.zeros((N_WF, 8), np.float32))
        with pytest.raises(ValueError, match="^inl_correction: inl holds at least one value$"):
            processors.inl_correction(_rows(np.uint16), np.zeros(0, np.float32))
        with pytest.raises(ValueError, match="^inl_correction: the output has the length of the input \\(len\\(w_in\\) = 16, len\\(w_out\\) = 17\\)$"):
            processors.inl_correction(_rows(np.uint16), np.zeros(8, np.float32), np.zeros((N_WF, LEN + 1), np.float32))
        for g, args in ((processors.get_wf_centroid, (0.0,)), (processors.wf_correction, (np.zeros(4), 0, 2))):
            with pytest.raises(NotImplementedError, match="the float64 loop takes float64 rows on the device$"):
                g(_rows(np.int32), *args)
        for shift, text in ((np.nan, "shift is nan"), (-1, "shift must be positive"), (15.5, "shift must be shorter than input waveform size")):
            with pytest.raises(DSPFatal, match=f"(?m)^{text}$"):
                processors.get_wf_centroid(w, shift)
        with pytest.raises(NotImplementedError, match="^get_wf_centroid: shift is a constant of the call on the device, not a per-event value$"):
            processors.get_wf_centroid(w, np.array([1.0, 2.0, 3.0]))
        for (shift, size), text in (((np.nan, np.nan), "shift is nan"), ((-1, -1), "shift must be positive"), ((16.5, 4), "shift must be shorter than input waveform size"),
                                    ((0, np.nan), "size is nan"), ((0, 0), "size must be positive"), ((0, 17), "size must be shorter than input waveform size")):
            with pytest.raises(DSPFatal, match=f"(?m)^{text}$"):
                processors.wf_alignment(w, 5.0, shift, size, out)
        processors.wf_alignment(w, 5.0, 16.0, 4, out)  # (shift == len(w_in) passes: the reference compares with >)
        del fake.calls[:]
        for size in (3, 4.5):
            with pytest.raises(ValueError, match=f"^wf_alignment: size is a whole number and equals len\\(w_out\\) \\(size = {size:g}, len\\(w_out\\) = 4\\)$"):
                processors.wf_alignment(w, 5.0, 0, size, out)
        with pytest.raises(DSPFatal, match="(?m)^centroid is nan$"):  # a constant: raised at the call, whatever the rows hold
            processors.wf_alignment(np.full((N_WF, LEN), np.nan, np.float32), np.nan, 0, 4, out)
        for k, name in ((2, "shift"), (3, "size")):
            args = [w, 5.0, 0.0, 4, out]
            args[k] = np.array([1.0, 2.0, 3.0])
            with pytest.raises(NotImplementedError, match=f"^wf_alignment: {name} is a constant of the call on the device, not a per-event value$"):
                processors.wf_alignment(*args)
        with pytest.raises(TypeError, match="w_out must be passed"):
            processors.wf_alignment(w, 5.0, 0.0, 4)
        for n, m, start, stop, text in ac.CORRECTION_REFUSALS:
            with pytest.raises(DSPFatal, match=f"(?m)^{text}$"):
                processors.wf_correction(np.zeros((2, n), np.float32), np.zeros(m), start, stop)
        with pytest.raises(NotImplementedError, match="^wf_correction: w_corr is one constant array of the call on the device, not an array per event$"):
            processors.wf_correction(w, np.zeros((N_WF, 4)), 0, 2)
        with pytest.raises(ValueError, match="^wf_correction: the output has the length of the input \\(len\\(w_in\\) = 16, len\\(w_out\\) = 4\\)$"):
            processors.wf_correction(w, np.zeros(4), 0, 2, out)
        assert fake.calls == [] and fake.live() == 0


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _table(dtype=np.uint16, n_rows=24, n=1000):
    from dspeed_amd.processing_chain import WaveformInput

    w = (1000 + (np.arange(n_rows * n).reshape(n_rows, n) * 7) % 41).astype(dtype)
    return {"waveform": WaveformInput(w, 16.0), "c_in": np.full(n_rows, 400, np.float32), "where": np.full(n_rows, 20, np.int32),
            "tpl_rows": np.zeros((n_rows, 100), np.float32)}


def _recipe(module=M, **changes):
    """the chain of the issue: every processor under the package's string, or under its file's"""
    mod = (lambda file: M) if module == M else (lambda file: f"{M}.{file}")
    procs = {
        "wf_inl": {"function": "inl_correction", "module": mod("inl_correction"), "args": ["waveform", "db.inl", "wf_inl"]},
        "kern_step": {"function": "step", "module": mod("kernels"), "args": [16, "kern_step(16, 'f')"]},
        "wf_step": {"function": "convolve_wf", "module": M, "args": ["wf_inl", "kern_step", "'s'", "wf_step(1000, 'f')"]},
        "centroid": {"function": "get_wf_centroid", "module": mod("get_wf_centroid"), "args": ["wf_step", 8, "centroid"]},
        "wf_align": {"function": "wf_alignment", "module": mod("wf_alignment"), "args": ["wf_inl", "centroid", 8, 200, "wf_align(200)"]},
        "wf_corr": {"function": "wf_correction", "module": mod("wf_correction"), "args": ["wf_align", "db.tpl", 20, 120, "wf_corr"]},
    }
    for key, args in changes.items():
        procs[key]["args"] = args
    return procs


DB = {"inl": [0.25 * (i % 5) for i in range(65536)], "tpl": [0.5 * i for i in range(100)]}


def _build(procs, outputs, table=None, db=DB):
    from dspeed_amd.processing_chain import build_processing_chain

    return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table(), db_dict=db)


FUSED = "wf_alignment wf_align + wf_correction wf_corr in one launch on rows"


def test_the_chain_of_the_issue_runs_from_a_recipe_to_wf_corr():
    for module in (M, "files"):
        chain, _, out = _build(_recipe(module), ["wf_corr"])
        mine = [s for s in _stages(chain) if s[1] == KERNEL]
        assert mine == [("inl_correction wf_inl on rows", KERNEL, [L, IN, ST]), ("get_wf_centroid centroid on rows", KERNEL, [L, CE, SS]), (FUSED, KERNEL, [L, AL, CO, ST])]
        whats = [s[0] for s in _stages(chain)]
        assert whats.index("inl_correction wf_inl on rows") < whats.index("wf_step -> HBM") < whats.index("get_wf_centroid centroid on rows") < whats.index(FUSED)
        assert not any(op[0] in (IN, CE, AL, CO) for op in chain._program.ops)
        assert out["wf_corr"].shape == (24, 200) and out["wf_corr"].dtype == np.float32
        inl, cen, fused = (next(st for st in chain._stages if st["what"] == w) for w in (mine[0][0], mine[1][0], FUSED))
        assert [(i[1], i[2]) for i in inl["program"].io if i[1] == _lib.IO_WF_IN] == [(_lib.IO_WF_IN, _lib.U16)]  # the raw column, as it lies in the table
        (table,) = [v for k, v in inl["consts"].items() if k.startswith("taps:")]
        assert table.dtype == np.float32 and np.array_equal(table, np.asarray(DB["inl"], np.float32))  # the float64 list, cast once on the host
        assert cen["program"].ops[1][5][0].kind == _lib.ARG_CONST and cen["program"].ops[1][5][0].value == 8.0
        sp = fused["program"].ops[1][5]
        assert sp[0].kind == _lib.ARG_INPUT and [s.value for s in sp[1:]] == [8.0, 200.0]  # the centroid: the column the stage ahead wrote
        assert fused["program"].ops[2][4][:2] == (20, 120) and [o[0] for o in fused["outs"]] == ["out:wf_corr"]  # no aligned row
        (tpl,) = [v for k, v in fused["consts"].items() if k.startswith("taps:")]
        assert np.array_equal(tpl, np.asarray(DB["tpl"], np.float32))
        # the step kernel ran at chain build
        (kern,) = [v for st in chain._stages for k, v in st["consts"].items() if k.startswith("taps:kern_step")]
        assert np.array_equal(kern[:16], ac.emulate_step(16))


def test_the_aligned_row_is_written_only_when_asked_for_or_read():
    chain, _, out = _build(_recipe(), ["wf_corr", "wf_align"])
    assert [s[2] for s in _stages(chain) if s[0] == FUSED] == [[L, AL, CO, ST, ST]] and out["wf_align"].shape == (24, 200)
    procs = _recipe()
    procs["a_max"] = {"function": "amax", "module": "numpy", "args": ["wf_align", 1, "a_max"]}  # another reader of the aligned row
    chain, _, out = _build(procs, ["wf_corr", "a_max"])
    assert [s[2] for s in _stages(chain) if s[0] == FUSED] == [[L, AL, CO, ST, ST]]
    # apart: the alignment alone; a correction of rows that are no alignment's
    chain, _, out = _build({k: v for k, v in _recipe().items() if k != "wf_corr"}, ["wf_align"])
    assert ("wf_alignment wf_align on rows", KERNEL, [L, AL, ST]) in _stages(chain)
    chain, _, out = _build(_recipe(wf_corr=["wf_inl", "db.tpl", 0, 100, "wf_corr"]), ["wf_corr", "wf_align"])
    mine = [s for s in _stages(chain) if s[1] == KERNEL]
    assert ("wf_alignment wf_align on rows", KERNEL, [L, AL, ST]) in mine and ("wf_correction wf_corr on rows", KERNEL, [L, CO, ST]) in mine
    assert out["wf_corr"].shape == (24, 1000)


def test_the_centroid_may_be_a_stage_result_an_input_column_or_a_constant():
    chain, _, out = _build(_recipe(wf_align=["wf_inl", "c_in", 8, 200, "wf_align(200)"]), ["wf_align"])
    (st,) = [s for s in chain._stages if s["what"] == "wf_alignment wf_align on rows"]
    assert st["program"].ops[1][5][0].kind == _lib.ARG_INPUT and not any(s["what"].startswith("get_wf_centroid") for s in chain._stages)
    chain, _, out = _build(_recipe(wf_align=["wf_inl", 400, 8, 200, "wf_align(200)"]), ["wf_align"])
    (st,) = [s for s in chain._stages if s["what"] == "wf_alignment wf_align on rows"]
    assert st["program"].ops[1][5][0].kind == _lib.ARG_CONST and st["program"].ops[1][5][0].value == 400.0
    # the raw integer rows aligned: the window alone is read
    chain, _, out = _build(_recipe(wf_align=["waveform", 400, 8, 200, "wf_align(200)"]), ["wf_align"])
    (st,) = [s for s in chain._stages if s["what"] == "wf_alignment wf_align on rows"]
    assert [(i[2], i[3]) for i in st["program"].io if i[1] == _lib.IO_WF_IN] == [(_lib.U16, 1000)]
    # the window's length from size, where the declaration gives none
    chain, _, out = _build(_recipe(wf_align=["wf_inl", 400, 8, 64, "wf_align"], wf_corr=["wf_align", "db.tpl", 0, 64, "wf_corr"]), ["wf_corr"])
    assert out["wf_corr"].shape == (24, 64)
    # the tables as list literals and as recipe entries holding one
    procs = _recipe(wf_corr=["wf_align", "[0.5, 1.5, 2.5]", 4, 7, "wf_corr"])
    chain, _, out = _build(procs, ["wf_corr"])
    (tpl,) = [v for s in chain._stages if s["what"] == FUSED for k, v in s["consts"].items() if k.startswith("taps:")]
    assert np.array_equal(tpl, np.array([0.5, 1.5, 2.5], np.float32))


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import WaveformInput

    for dtype in (np.float64, np.int32):
        tb64 = dict(_table(dtype, 4, 100))
        with pytest.raises(NotImplementedError, match="(inl_correction|get_wf_centroid|wf_alignment|wf_correction) in a recipe whose loop type is float64"):
            _build(_recipe(), ["wf_corr"], tb64)
    tbf = {"waveform": WaveformInput(np.full((4, 1000), 1000.0, np.float32), 16.0)}
    with pytest.raises(NotImplementedError, match="inl_correction \\(wf_inl\\): 'waveform' is not an integer input column: inl_correction reads ADC codes"):
        _build(_recipe(), ["wf_inl"], tbf)
    procs = _recipe()
    procs["wf_bl"] = {"function": "bl_subtract", "module": M, "args": ["waveform", 5.0, "wf_bl"]}
    procs["wf_inl"]["args"][0] = "wf_bl"
    with pytest.raises(NotImplementedError, match="inl_correction \\(wf_inl\\): 'wf_bl' is not an integer input column"):
        _build(procs, ["wf_inl"])
    with pytest.raises(NotImplementedError, match="inl_correction \\(wf_inl\\): inl is one constant array of the call on the device, not an array per event"):
        _build(_recipe(wf_inl=["waveform", "tpl_rows", "wf_inl"]), ["wf_inl"])
    with pytest.raises(NotImplementedError, match="wf_correction \\(wf_corr\\): w_corr is one constant array of the call on the device, not an array per event"):
        _build(_recipe(wf_corr=["wf_align", "tpl_rows", 20, 120, "wf_corr"]), ["wf_corr"])
    with pytest.raises(NotImplementedError, match="get_wf_centroid \\(centroid\\): shift is a constant of the call on the device, not a per-event value"):
        _build(_recipe(centroid=["wf_step", "c_in", "centroid"]), ["centroid"])
    for k, name in ((2, "shift"), (3, "size")):
        args = ["wf_inl", "centroid", 8, 200, "wf_align(200)"]
        args[k] = "c_in"
        with pytest.raises(NotImplementedError, match=f"wf_alignment \\(wf_align\\): {name} is a constant of the call on the device, not a per-event value"):
            _build(_recipe(wf_align=args), ["wf_align"])
    # the checks of the constants, in the reference's words, at chain build
    with pytest.raises(DSPFatal, match="(?m)^shift must be shorter than input waveform size$"):
        _build(_recipe(centroid=["wf_step", 1000, "centroid"]), ["centroid"])
    with pytest.raises(DSPFatal, match="(?m)^size must be shorter than input waveform size$"):
        _build(_recipe(wf_align=["wf_inl", "centroid", 8, 1001, "wf_align(1001)"]), ["wf_align"])
    with pytest.raises(ProcessingChainError, match="wf_alignment \\(wf_align\\): size is a whole number and equals len\\(w_out\\) \\(size = 200, len\\(w_out\\) = 100\\)"):
        _build(_recipe(wf_align=["wf_inl", "centroid", 8, 200, "wf_align(100)"]), ["wf_align"])
    with pytest.raises(DSPFatal, match="(?m)^stop_idx must be shorter than input waveform size$"):  # (of the window: 200 samples)
        _build(_recipe(wf_corr=["wf_align", "db.tpl", 150, 201, "wf_corr"]), ["wf_corr"])
    with pytest.raises(DSPFatal, match="(?m)^stop_idx - start_idx must be smaller than len\\(w_corr\\)$"):
        _build(_recipe(wf_corr=["wf_align", "db.tpl", 20, 121, "wf_corr"]), ["wf_corr"])
    with pytest.raises(DSPFatal, match="(?m)^centroid is nan$"):
        _build(_recipe(wf_align=["wf_inl", "db.c_nan", 8, 200, "wf_align(200)"]), ["wf_align"], db=dict(DB, c_nan=float("nan")))
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="(inl_correction|get_wf_centroid|wf_alignment|wf_correction) runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        _build(_recipe(), ["wf_corr"])
