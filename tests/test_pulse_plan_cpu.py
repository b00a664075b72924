"""The planner's, the registry's and the recipe compiler's part of the pulse picker without a device (dsp_chain_plan):
DSP_OP_PEAK_SNR_THRESHOLD and DSP_OP_MULTI_A_FILTER have one route -- dsp_pulses_kernel, whatever the switches say --, three program shapes
and every refusal by name; the opcodes are appended; the two processors are attributes of the registry listed in ``PULSES``; what a call
hands to the library (against a subclass of tests/fake_dsp_lib.FakeLib); the stages of the SiPM recipe
reflected_convolve_wf -> avg_current -> histogram + histogram_stats -> get_multi_local_extrema -> peak_snr_threshold -> multi_a_filter."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import fake_dsp_lib
import pulse_cases as pc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import DSPFatal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = pc.KERNEL
F64 = dict(rows=np.float64, loop=np.float64)
L, PK, MA, ST, SS = _lib.OP_LOAD, _lib.OP_PEAK_SNR_THRESHOLD, _lib.OP_MULTI_A_FILTER, _lib.OP_STORE, _lib.OP_STORE_SCALAR
ROUTE = "DSP_OP_PEAK_SNR_THRESHOLD / DSP_OP_MULTI_A_FILTER \\(peak_snr_threshold, multi_a_filter\\) run on dsp_pulses_kernel only, on rows in memory: "
SHAPES = (ROUTE + "the program must be exactly LOAD, LOAD of the list, PEAK_SNR_THRESHOLD, STORE, STORE_SCALAR; or LOAD, LOAD of the list, MULTI_A_FILTER, "
          "STORE; or LOAD, LOAD of the list, PEAK_SNR_THRESHOLD, MULTI_A_FILTER, \\[STORE of idx_out,\\] STORE of va_max_out, STORE_SCALAR")


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_three_shapes_take_the_pulses_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for n in pc.LENGTHS + (8192,):
            for m in pc.LIST_LENGTHS:
                assert plan(pc.program(n, m))["kernel"] == KERNEL and plan(pc.program(n, m, **F64), np.float64)["kernel"] == KERNEL
                if m < n:
                    for kw in (dict(pick=False, amp=True), dict(amp=True), dict(amp=True, store_list=False)):
                        assert plan(pc.program(n, m, **kw))["kernel"] == KERNEL and plan(pc.program(n, m, **kw, **F64), np.float64)["kernel"] == KERNEL
        for rows in (np.int16, np.uint16):
            assert plan(pc.program(1000, rows=rows, amp=True))["kernel"] == KERNEL
            assert plan(pc.program(1000, 30, rows=rows, offset=3, row_stride=1007, list_offset=2, list_stride=37, out_stride=33, amp=True))["kernel"] == KERNEL
        assert plan(pc.program(1000, ratio="column"))["kernel"] == KERNEL and plan(pc.program(1000, ratio=float("nan"), amp=True))["kernel"] == KERNEL
        for width in (0, 0.5, 10, 1000, 1e9, 1e300):  # (a width beyond the row is clamped to it)
            assert plan(pc.program(1000, width=width))["kernel"] == KERNEL
        assert [op[0] for op in pc.program(64, amp=True).ops] == [L, L, PK, MA, ST, ST, SS]
        assert [op[0] for op in pc.program(64, amp=True, store_list=False).ops] == [L, L, PK, MA, ST, SS]
        assert [op[0] for op in pc.program(64, pick=False, amp=True).ops] == [L, L, MA, ST] and [op[0] for op in pc.program(64).ops] == [L, L, PK, ST, SS]
        p = pc.program(64, amp=True)
        p.ops[0], p.ops[1] = p.ops[1], p.ops[0]  # the two loads in either order
        assert plan(p)["kernel"] == KERNEL

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_limits_the_case_book_assumes_are_the_headers():
    program_h = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_program.h")).read()
    assert "#define DSP_PEAKS_MAX 64" in program_h and _lib.PEAKS_MAX == 64 == _lib.THRESH_MAX
    kernels_h = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    mine = kernels_h[kernels_h.index("namespace dsp_pulses {"):kernels_h.index("}  // namespace dsp_pulses")]
    assert "constexpr Window window(double idx, int n, int width)" in mine and "constexpr bool dropped(double idx, int n)" in mine
    assert max(pc.LIST_LENGTHS) == 64 and {63, 64} <= set(pc.LIST_LENGTHS) and {64, 65} <= set(pc.LENGTHS)


def test_any_other_program_with_the_ops_is_refused_by_name():
    p = pc.program(1000)
    p.ops.pop()  # the count not stored
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000, amp=True)
    p.ops.pop(4), p.ops.pop(4)  # nothing stored but the count
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))
    with pytest.raises(NotImplementedError, match=SHAPES):  # an intermediate as the source: rows in memory only
        plan(p)
    p = pc.program(1000, amp=True)
    p.ops.insert(3, p.ops[2])  # two pickers
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000, amp=True)
    p.add_op(ST, src=2, io=p.add_io("again", _lib.IO_WF_OUT, np.float32, 20, 0, None))  # a store behind the count
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = pc.program(1000, amp=True)
    p.ops[3] = p.ops[3][:4] + ((1,),) + p.ops[3][5:]  # the pick-off of the list as loaded beside a picker
    with pytest.raises(NotImplementedError, match=ROUTE + "multi_a_filter in the same program reads the same row at exactly the picker's idx_out"):
        plan(p)
    p = pc.program(1000, amp=True)
    p.ops[5] = p.ops[4]  # idx_out stored twice, the amplitudes never
    with pytest.raises(NotImplementedError, match=ROUTE + "idx_out and va_max_out are stored once each, whole, in the loop's type; the count once, into a DSP_U32 column"):
        plan(p)
    with pytest.raises(NotImplementedError, match=ROUTE + "idx_out and va_max_out are stored once each.*the count once, into a DSP_U32 column"):
        plan(pc.program(1000, count_type=np.float32))
    p = pc.program(1000)
    p.io[1] = p.io[1][:2] + (_lib.I16,) + p.io[1][3:]  # the list in another type than the loop's
    with pytest.raises(NotImplementedError, match=ROUTE + "the list is loaded whole into slot ip\\[0\\], a list per row in the loop's type"):
        plan(p)
    for rows in (np.int32, np.uint32):
        with pytest.raises(NotImplementedError, match=ROUTE + "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(pc.program(1000, rows=rows, loop=np.float64), np.float64)
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(pc.program(1000, rows=np.float64, loop=np.float32))


def test_the_planners_argument_errors():
    for m in (65, 100, 1000):
        with pytest.raises(NotImplementedError, match=f"peak_snr_threshold: at most 64 candidates \\({m} given\\): a wavefront keeps one per lane"):
            plan(pc.program(2000, m))
        with pytest.raises(NotImplementedError, match=f"multi_a_filter: at most 64 positions \\({m} given\\): a wavefront keeps one per lane"):
            plan(pc.program(2000, m, pick=False, amp=True))
    with pytest.raises(NotImplementedError, match="peak_snr_threshold: width_in is a constant of the program, not a per-event value"):
        plan(pc.program(1000, width="column"))
    for width in (-1, -0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="peak_snr_threshold: width_in is a non-negative number of samples"):
            plan(pc.program(1000, width=width))
    for n, m in ((20, 20), (3, 20), (2, 2), (64, 64)):
        for kw in (dict(pick=False, amp=True), dict(amp=True)):
            with pytest.raises(DSPFatal, match="^The length of your return array must be smaller than the length of your waveform"):
                plan(pc.program(n, m, **kw))
        assert plan(pc.program(n, m))["kernel"] == KERNEL  # the picker has no such rule
    with pytest.raises(ValueError, match="peak_snr_threshold: idx_out has the length of idx_in \\(19 and 20\\)"):
        plan(pc.program(1000, out_len=19))
    with pytest.raises(ValueError, match="multi_a_filter: va_max_out has the length of vt_maxs_in \\(21 and 20\\)"):
        plan(pc.program(1000, pick=False, amp=True, amp_len=21))
    p = pc.program(1000)
    p.ops[2] = p.ops[2][:1] + (1,) + p.ops[2][2:]  # idx_out in the slot of idx_in
    with pytest.raises(ValueError, match="bad PEAK_SNR_THRESHOLD \\(src: the slot of the row; ip\\[0\\]: the slot of idx_in; dst: another slot, for idx_out; ip\\[1\\]: the register of the count\\)"):
        plan(p)
    p = pc.program(1000, pick=False, amp=True)
    p.ops[2] = p.ops[2][:2] + (1,) + p.ops[2][3:]  # the list as the row
    with pytest.raises(ValueError, match="bad MULTI_A_FILTER \\(src: the slot of the row; ip\\[0\\]: the slot of vt_maxs_in; dst: another slot, for va_max_out\\)"):
        plan(p)
    assert _lib.fatal_message(36) == "The length of your return array must be smaller than the length of your waveform"


def test_the_opcodes_are_appended_and_the_registry_lists_the_processors_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _PROCESSOR_FILES, _PULSE_FILES, _SIGS, module_accepted

    assert (_lib.OP_BI_LEVEL_ZERO_CROSSING, _lib.OP_PEAK_SNR_THRESHOLD, _lib.OP_MULTI_A_FILTER) == (47, 48, 49)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_PEAK_SNR_THRESHOLD 48" in header and "#define DSP_OP_MULTI_A_FILTER 49" in header and "#define DSP_E_MAF_LEN 36" in header
    assert "dsp_peak_snr_threshold_f32" not in header and "dsp_multi_a_filter_f32" not in header  # (one entry each, the loop an argument)
    assert processors.PULSES == ("peak_snr_threshold", "multi_a_filter")
    others = (set(processors.__all__) | set(processors.SPECTRAL) | set(processors.ORDER) | set(processors.RESAMPLING) | set(processors.ML)
              | set(processors.SMOOTHING) | set(processors.PILEUP) | set(_PROCESSOR_FILES))
    assert not set(processors.PULSES) & others
    g = processors.peak_snr_threshold
    assert g.signature == "(n),(m),(),()->(m),()" and g.types == ["ffff->fI", "dddd->dI"] and (g.nin, g.nout, g.nargs) == (4, 2, 6) and g.__name__ == "peak_snr_threshold"
    g = processors.multi_a_filter
    assert g.signature == "(n),(m)->(m)" and g.types == ["ff->f", "dd->d"] and (g.nin, g.nout, g.nargs) == (2, 1, 3) and g.__name__ == "multi_a_filter"
    assert _SIGS["peak_snr_threshold"] == "wwssWS" and _SIGS["multi_a_filter"] == "wwW"
    assert _PULSE_FILES == {"peak_snr_threshold": ("peak_snr_threshold",), "multi_a_filter": ("multi_a_filter",)}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for entry in ("dsp_peak_snr_threshold_rows", "dsp_multi_a_filter_rows"):
        assert hasattr(lib, entry) and entry in _lib.EXPORTS
    for fn in processors.PULSES:  # the config's module strings
        assert module_accepted(M, fn) and module_accepted(f"{M}.{fn}", fn) and module_accepted("dspeed_amd.processors", fn)
    assert not module_accepted(f"{M}.multi_a_filter", "peak_snr_threshold") and not module_accepted(f"{M}.peak_snr_threshold", "multi_a_filter")


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entries that name their loop in an argument instead of a suffix"""

    def dsp_peak_snr_threshold_rows(self, *args):
        self.calls.append(["dsp_peak_snr_threshold_rows"] + [self._name(a) for a in args])
        return 0

    def dsp_multi_a_filter_rows(self, *args):
        self.calls.append(["dsp_multi_a_filter_rows"] + [self._name(a) for a in args])
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
def test_the_arguments_of_a_picker_call(dtype, code, loop_code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, the list (pointer, length, stride), the ratio as (column or NULL,
    constant), the width, idx_out and its stride, the count, the stream, the row of an error"""
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    lists = np.arange(N_WF * LISTS).reshape(N_WF, LISTS) % LEN
    with _installed() as fake:
        idx, count = processors.peak_snr_threshold(_rows(dtype), lists, 0.8, 10)  # the outputs left out: new arrays, m of the list
        assert idx.shape == (N_WF, LISTS) and idx.dtype == loop and count.shape == (N_WF,) and count.dtype == np.uint32
        (call,) = fake.calls
        assert call[0] == "dsp_peak_snr_threshold_rows" and len(call) == 18
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == ["ptr", 1, 0, N_WF * LISTS * esz] and call[8:10] == [LISTS, LISTS] and call[10:12] == [None, 0.8] and call[12] == 10.0
        assert call[13] == ["ptr", 2, 0, N_WF * LISTS * esz] and call[14] == LISTS and call[15] == ["ptr", 3, 0, N_WF * 4]
        assert call[16] is None and call[17] == "byref" and fake.live() == 0
        del fake.calls[:]
        # one list for every row; a ratio per row; the outputs passed: written in place, returned
        oi, oc = np.zeros((N_WF, LISTS), loop), np.zeros(N_WF, np.uint32)
        got = processors.peak_snr_threshold(_rows(dtype), lists[0], np.array([0.5, 0.6, 0.7]), np.float32(3.9), oi, oc)
        assert got[0] is oi and got[1] is oc
        (call,) = fake.calls
        assert call[8:10] == [LISTS, LISTS] and call[10][0] == "ptr" and call[10][2:] == [0, N_WF * esz] and call[12] == pytest.approx(3.9)
        del fake.calls[:]
        idx, count = processors.peak_snr_threshold(_rows(dtype, (LEN,)), lists[0], 0.8, 2)  # a 1-D call
        assert idx.shape == (LISTS,) and np.ndim(count) == 0 and np.asarray(count).dtype == np.uint32
        (call,) = fake.calls
        assert call[2:6] == [code, 1, LEN, LEN] and call[8:10] == [LISTS, LISTS]
        # rows, list and outputs on the device: their own memory, nothing staged
        d, dl = DeviceArray.from_numpy(_rows(dtype)), DeviceArray.from_numpy(lists.astype(loop))
        do, dc = DeviceArray((N_WF, LISTS), loop), DeviceArray((N_WF,), np.uint32)
        before = len(fake.device)
        got = processors.peak_snr_threshold(d, dl, 0.8, 10, do, dc)
        assert got[0] is do and got[1] is dc and len(fake.device) == before
        assert [fake.calls[-1][k][1] for k in (1, 7, 13, 15)] == [before - 4, before - 3, before - 2, before - 1]
        for x in (d, dl, do, dc):
            x.free()
        assert fake.live() == 0


@pytest.mark.parametrize("dtype, code, loop_code, loop", CALLS)
def test_the_arguments_of_a_pickoff_call(dtype, code, loop_code, loop):
    from dspeed_amd import processors

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    lists = np.arange(N_WF * LISTS).reshape(N_WF, LISTS) % LEN
    with _installed() as fake:
        amp = processors.multi_a_filter(_rows(dtype), lists)
        assert amp.shape == (N_WF, LISTS) and amp.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_multi_a_filter_rows" and len(call) == 14
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == ["ptr", 1, 0, N_WF * LISTS * esz] and call[8:10] == [LISTS, LISTS] and call[10] == ["ptr", 2, 0, N_WF * LISTS * esz]
        assert call[11] == LISTS and call[12] is None and call[13] == "byref" and fake.live() == 0
        del fake.calls[:]
        out = np.zeros(LISTS, loop)
        assert processors.multi_a_filter(_rows(dtype, (LEN,)), lists[0], out) is out  # a 1-D call, the output passed
        assert fake.calls[0][2:6] == [code, 1, LEN, LEN]


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors

    pick, amp = processors.peak_snr_threshold, processors.multi_a_filter
    lists = np.zeros((N_WF, LISTS))
    with _installed() as fake:
        with pytest.raises(NotImplementedError, match="^peak_snr_threshold: the float64 loop takes float64 rows on the device$"):
            pick(_rows(np.int32), lists, 0.8, 10)
        with pytest.raises(NotImplementedError, match="^multi_a_filter: the float64 loop takes float64 rows on the device$"):
            amp(_rows(np.uint32), lists)
        with pytest.raises(NotImplementedError, match="^peak_snr_threshold: per-waveform integer parameters are not supported on the device$"):
            pick(_rows(np.float32), lists, 0.8, np.array([10, 11, 12]))
        for width in (-1, -0.25, np.nan, np.inf):
            with pytest.raises(ValueError, match="^peak_snr_threshold: width_in is a non-negative number of samples$"):
                pick(_rows(np.float32), lists, 0.8, width)
        with pytest.raises(NotImplementedError, match="^peak_snr_threshold: at most 64 list entries \\(65 given\\): a wavefront keeps one per lane$"):
            pick(np.zeros((2, 100), np.float32), np.zeros((2, 65)), 0.8, 10)
        with pytest.raises(NotImplementedError, match="^multi_a_filter: at most 64 list entries \\(65 given\\): a wavefront keeps one per lane$"):
            amp(np.zeros((2, 100), np.float32), np.zeros((2, 65)))
        for m in (LEN, LEN + 1):
            with pytest.raises(DSPFatal, match="^The length of your return array must be smaller than the length of your waveform$"):
                amp(_rows(np.float32), np.zeros((N_WF, m)))
        with pytest.raises(ValueError, match="^peak_snr_threshold: the output has the length of the list \\(5 entries, 4 given\\)$"):
            pick(_rows(np.float32), lists, 0.8, 10, np.zeros((N_WF, 4), np.float32), None)
        with pytest.raises(ValueError, match="^multi_a_filter: the output has the length of the list \\(5 entries, 6 given\\)$"):
            amp(_rows(np.float32), lists, np.zeros((N_WF, 6), np.float32))
        with pytest.raises(ValueError, match="^peak_snr_threshold: idx_in has shape \\(2, 5\\), expected \\(3, m\\) or \\(m,\\)$"):
            pick(_rows(np.float32), np.zeros((2, LISTS)), 0.8, 10)
        with pytest.raises(TypeError, match="takes 4 inputs and 2 outputs"):
            pick(_rows(np.float32), lists, 0.8)
        with pytest.raises(TypeError, match="takes 2 inputs and 1 outputs"):
            amp(_rows(np.float32))
        # an empty list: empty outputs, counts of zero, no launch
        idx, count = pick(_rows(np.float32), np.zeros((N_WF, 0)), 0.8, 10)
        assert idx.shape == (N_WF, 0) and idx.dtype == np.float32 and list(count) == [0, 0, 0] and count.dtype == np.uint32
        oc = np.full(N_WF, 7, np.uint32)
        assert pick(_rows(np.float32), np.zeros((N_WF, 0)), 0.8, 10, np.zeros((N_WF, 0), np.float32), oc)[1] is oc and list(oc) == [0, 0, 0]
        assert amp(_rows(np.float64), np.zeros((N_WF, 0))).shape == (N_WF, 0)
        assert fake.calls == [] and fake.live() == 0


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _table(n_rows=24, n=1000):
    from dspeed_amd.processing_chain import WaveformInput

    w = (1000 + (np.arange(n_rows * n).reshape(n_rows, n) * 7) % 41).astype(np.uint16)
    return {"waveform": WaveformInput(w, 16.0), "ratios": np.full(n_rows, 0.8, np.float32), "cands": np.zeros((n_rows, 20), np.float32)}


PEAKS = "vt_max_candidate_out, vt_min_out, n_max_out, n_min_out"
PICK, STATS, HIST = "trigger_pos, no_out", "fwhm, idx_out_c, max_out", "hist_weights, hist_borders"


def _sipm(ratio=0.8, width=10, trigger="trigger_pos(vector_len=no_out)", energies="energies(vector_len=len(trigger_pos))", amp_of="curr", unit="ns"):
    """the SiPM config's entries behind gaussian_filter1d, as it writes them; the Gaussian weights come as db.kernel"""
    return {
        "wf_gaus": {"function": "reflected_convolve_wf", "module": f"{M}.convolutions", "args": ["waveform", "db.kernel", "wf_gaus"], "unit": "ADC"},
        "curr": {"function": "avg_current", "module": f"{M}.moving_windows", "args": ["wf_gaus", 5, "curr(len(wf_gaus)-5, period=waveform.period)"], "unit": "ADC"},
        HIST: {"function": "histogram", "module": f"{M}.histogram", "args": ["curr", "hist_weights(100)", "hist_borders(101)"], "unit": ["none", "ADC"]},
        STATS: {"function": "histogram_stats", "module": M, "args": ["hist_weights", "hist_borders", "idx_out_c", "max_out", "fwhm", "np.nan"],
                "unit": ["ADC", "non", "ADC"]},
        PEAKS: {"function": "get_multi_local_extrema", "module": f"{M}.get_multi_local_extrema",
                "args": ["curr", 5, 0.1, 1, "3*fwhm", 0, "vt_max_candidate_out(20, vector_len=n_max_out)", "vt_min_out(20, vector_len=n_min_out)", "n_max_out", "n_min_out"],
                "unit": ["ns", "ns", "none", "none"]},
        PICK: {"function": "peak_snr_threshold", "module": f"{M}.peak_snr_threshold",
               "args": ["curr", "vt_max_candidate_out", ratio, width, trigger, "no_out"], "unit": [unit, "none"]},
        "energies": {"function": "multi_a_filter", "module": f"{M}.multi_a_filter", "args": [amp_of, "trigger_pos", energies], "unit": ["ADC"]},
    }


def _build(procs, outputs, table=None):
    from dspeed_amd.processing_chain import build_processing_chain
    from dspeed_amd.processors import gaussian_filter1d

    k = gaussian_filter1d(np.float32(1), np.float32(4), np.empty(9, np.float32))
    return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table(), db_dict={"kernel": k})


FUSED = f"peak_snr_threshold {PICK} + multi_a_filter energies in one launch on rows"


def test_the_sipm_fragment_is_staged_in_the_order_the_data_flows():
    chain, _, out = _build(_sipm(), ["energies", "trigger_pos"])  # the config's two outputs
    stages = _stages(chain)
    assert [(s[0], s[1]) for s in stages] == [
        ("reflected_convolve_wf wf_gaus + avg_current curr in one launch on rows", "dsp_reflect_kernel"),
        (f"histogram {HIST} + histogram_stats {STATS} in one launch on rows", "dsp_hist_kernel"),
        (f"(3*fwhm) for get_multi_local_extrema {PEAKS}", "dsp_scalar_kernel"),
        (f"get_multi_local_extrema {PEAKS} on rows", "dsp_extrema_kernel"),
        (FUSED, KERNEL)]
    assert stages[-1][2] == [L, L, PK, MA, ST, ST, SS]  # trigger_pos is asked for: stored
    (stage,) = [st for st in chain._stages if st["what"] == FUSED]
    assert [o[0] for o in stage["outs"]] == ["out:trigger_pos", "out:energies", "out:no_out"]
    pk = stage["program"].ops[2]
    assert pk[5][0].kind == _lib.ARG_CONST and pk[5][0].value == pytest.approx(0.8) and pk[5][1].kind == _lib.ARG_CONST and pk[5][1].value == 10.0
    assert [(i[3], i[4]) for i in stage["program"].io if i[1] == _lib.IO_WF_IN] == [(995, 0), (20, 0)]  # curr and the peak finder's list
    assert not any(op[0] in (PK, MA) for op in chain._program.ops)
    # the lengths are m of the list read: nothing in the declarations says 20
    assert out["trigger_pos"].shape == (24, 20) and out["energies"].shape == (24, 20) and out["energies"].dtype == np.float32
    assert chain.vector_lens == {"energies": "no_out", "trigger_pos": "no_out"} and chain.hidden_outputs == ["no_out"]
    # trigger_pos in ns: sample indices inside the chain, converted where the recipe's output is stored (an add and a multiply, as the peak finder's lists)
    assert [op[0] for op in chain._program.ops].count(_lib.OP_ELEMENTWISE) == 2
    chain, _, out = _build(_sipm(unit="none"), ["energies", "trigger_pos"])
    assert [op[0] for op in chain._program.ops].count(_lib.OP_ELEMENTWISE) == 0


def test_the_packed_list_is_stored_only_when_asked_for_or_read():
    chain, _, out = _build(_sipm(), ["energies"])
    assert _stages(chain)[-1] == (FUSED, KERNEL, [L, L, PK, MA, ST, SS])  # registers only
    assert chain.vector_lens == {"energies": "no_out"} and set(out) == {"energies", "no_out"} and out["no_out"].dtype == np.uint32
    # another reader of trigger_pos: written, and read from there; the launch stays fused
    procs = {**_sipm(), "t_first": {"function": "fixed_time_pickoff", "module": M, "args": ["trigger_pos", 0, "'i'", "t_first"]}}
    chain, _, out = _build(procs, ["energies", "t_first"])
    assert [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, L, PK, MA, ST, ST, SS]]
    # the pick-off on another waveform than the picker's: two launches, the list through memory
    chain, _, out = _build(_sipm(amp_of="wf_gaus[0:995]"), ["energies"])
    mine = [s for s in _stages(chain) if s[1] == KERNEL]
    assert [s[0] for s in mine] == [f"peak_snr_threshold {PICK} on rows", "multi_a_filter energies on rows"]
    assert [s[2] for s in mine] == [[L, L, PK, ST, SS], [L, L, MA, ST]]
    # the picker alone; the pick-off alone on the peak finder's list
    chain, _, out = _build(_sipm(), ["trigger_pos", "no_out"])
    assert _stages(chain)[-1] == (f"peak_snr_threshold {PICK} on rows", KERNEL, [L, L, PK, ST, SS]) and chain.hidden_outputs == []
    procs = {k: v for k, v in _sipm().items() if k != PICK}
    procs["energies"] = {"function": "multi_a_filter", "module": f"{M}.multi_a_filter", "args": ["curr", "vt_max_candidate_out", "energies(vector_len=n_max_out)"]}
    chain, _, out = _build(procs, ["energies"])
    assert _stages(chain)[-1] == ("multi_a_filter energies on rows", KERNEL, [L, L, MA, ST]) and chain.vector_lens == {"energies": "n_max_out"}


def test_a_ratio_per_event_and_a_list_from_the_table():
    procs = {PICK: {"function": "peak_snr_threshold", "module": f"{M}.peak_snr_threshold", "args": ["waveform", "cands", "ratios", 10, "trigger_pos(vector_len=no_out)", "no_out"]},
             "energies": {"function": "multi_a_filter", "module": f"{M}.multi_a_filter", "args": ["waveform", "trigger_pos", "energies(vector_len=no_out)"]}}
    chain, _, out = _build(procs, ["energies", "no_out"])
    assert _stages(chain) == [(FUSED, KERNEL, [L, L, PK, MA, ST, SS])]
    assert chain._stages[0]["program"].ops[2][5][0].kind == _lib.ARG_INPUT  # the ratio: the table's column
    procs[PICK]["args"][2] = "2*ratios"  # an expression: a small program of its own ahead of the launch
    chain, _, out = _build(procs, ["energies", "no_out"])
    assert [s[1] for s in _stages(chain)] == ["dsp_scalar_kernel", KERNEL]


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import WaveformInput

    with pytest.raises(NotImplementedError, match="peak_snr_threshold \\(trigger_pos, no_out\\): per-waveform integer parameters are not supported on the device"):
        _build(_sipm(width="ratios"), ["energies"])
    for width in (-1, "np.nan", "np.inf"):
        with pytest.raises(ValueError, match="peak_snr_threshold \\(trigger_pos, no_out\\): width_in is a non-negative number of samples"):
            _build(_sipm(width=width), ["energies"])
    with pytest.raises(ValueError, match="peak_snr_threshold \\(trigger_pos, no_out\\): the output has the length of the list \\(20 entries, 19 given\\)"):
        _build(_sipm(trigger="trigger_pos(19, vector_len=no_out)"), ["energies"])
    with pytest.raises(ValueError, match="multi_a_filter \\(energies\\): the output has the length of the list \\(20 entries, 21 given\\)"):
        _build(_sipm(energies="energies(21, vector_len=no_out)"), ["energies"])
    procs = _sipm()
    procs[PEAKS]["args"][6:8] = ["vt_max_candidate_out(65, vector_len=n_max_out)", "vt_min_out(65, vector_len=n_min_out)"]
    with pytest.raises(NotImplementedError, match="peak_snr_threshold \\(trigger_pos, no_out\\): at most 64 list entries \\(65 given\\): a wavefront keeps one per lane"):
        _build(procs, ["energies"])
    tb = {"waveform": WaveformInput(np.full((4, 20), 1000, np.uint16), 16.0), "cands": np.zeros((4, 20), np.float32)}
    procs = {"energies": {"function": "multi_a_filter", "module": f"{M}.multi_a_filter", "args": ["waveform", "cands", "energies"]}}
    with pytest.raises(DSPFatal, match="The length of your return array must be smaller than the length of your waveform"):
        _build(procs, ["energies"], tb)
    with pytest.raises(Exception, match="peak_snr_threshold"):
        _build({**_sipm(), PICK: {**_sipm()[PICK], "module": f"{M}.multi_a_filter"}}, ["energies"])  # not its file
    # under the package's module string both stay refused, in the words an existing test and the recorded translations hold: recipes name
    # the processors' files, as the SiPM configs do
    for fn, key in (("peak_snr_threshold", PICK), ("multi_a_filter", "energies")):
        for module in (M, "dspeed_amd.processors"):
            with pytest.raises(NotImplementedError, match=f"^processor '{fn}' is not implemented on the device path$"):
                _build({**_sipm(), key: {**_sipm()[key], "module": module}}, ["energies"])
    tb64 = {"waveform": WaveformInput(np.full((4, 100), 1000.0), 16.0), "cands": np.zeros((4, 20), np.float64)}
    with pytest.raises(NotImplementedError, match="(peak_snr_threshold|multi_a_filter) in a recipe whose loop type is float64"):
        _build(procs, ["energies"], tb64)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="(peak_snr_threshold|multi_a_filter) runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        _build(procs, ["energies"], tb)
