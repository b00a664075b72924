"""The planner's, the registry's and the recipe compiler's part of psd and fft without a device (dsp_chain_plan): DSP_OP_PSD and DSP_OP_FFT
have one route -- dsp_spectrum_kernel, whatever the switches say --, two program shapes and every refusal by name; the opcodes are appended;
the two processors are attributes of the registry listed in ``SPECTRAL``; what a call hands to the library (against
tests/fake_dsp_lib.py, recorded in tests/golden/spectrum_calls.json.gz by tools/record_spectrum_calls.py); the stage list of a recipe
with the reference's own declaration."""
import contextlib
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import fake_dsp_lib
import spectrum_cases as sc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import DSPFatal, ProcessingChainError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spectrum_calls.json.gz")
M = "dspeed.processors"
KERNEL = "dsp_spectrum_kernel"
LIMITS = "the float32 loop takes rows of a power of two up to 16384 samples and of any other length up to 4096"
LIMITS64 = "the float64 loop takes rows of a power of two up to 8192 samples and of any other length up to 2048"


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_shapes_take_the_spectrum_kernel_whatever_the_switches_say(monkeypatch):
    for op in ("psd", "fft"):
        for n in sc.LENGTHS:
            assert plan(sc.program(n, op))["kernel"] == KERNEL
            if sc.admitted(n, np.float64):
                assert plan(sc.program(n, op, np.float64, np.float64), np.float64)["kernel"] == KERNEL
        assert plan(sc.program(1000, op, np.int16))["kernel"] == KERNEL
        assert plan(sc.program(1000, op, np.uint16, offset=3, row_stride=1007))["kernel"] == KERNEL
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    assert plan(sc.program(1024))["kernel"] == KERNEL and plan(sc.program(1000, "fft"))["kernel"] == KERNEL


def test_the_length_check_comes_first_with_the_reference_s_texts():
    for op in ("psd", "fft"):
        for n, bins in ((1000, 500), (1000, 502), (1024, 512), (1, 2), (100000, 7)):  # (the last: before the limits)
            with pytest.raises(DSPFatal, match=f"Size of {op} must be len\\(w_in\\)//2\\+1 = {n // 2 + 1}$|Size of {op} must be len\\(w_in\\)//2\\+1 = {n // 2 + 1}\n"):
                plan(sc.program(n, op, bins=bins))
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.dsp_fatal_message.restype = ctypes.c_char_p
    assert [L.dsp_fatal_message(c).decode() for c in (33, 34)] == ["Size of fft must be len(w_in)//2+1", "Size of psd must be len(w_in)//2+1"]


def test_the_limits_by_name():
    for op in ("psd", "fft"):
        plan(sc.program(16384, op)), plan(sc.program(4096, op)), plan(sc.program(4095, op))
        for n in (4097, 5000, 16385, 32768, 1 << 19):
            with pytest.raises(NotImplementedError, match=f"{op}: {LIMITS} \\({n} given\\)"):
                plan(sc.program(n, op))
        plan(sc.program(8192, op, np.float64, np.float64), np.float64), plan(sc.program(2047, op, np.float64, np.float64), np.float64)
        for n in (2049, 3000, 16384):
            with pytest.raises(NotImplementedError, match=f"{op}: {LIMITS64} \\({n} given\\)"):
                plan(sc.program(n, op, np.float64, np.float64), np.float64)
    with pytest.raises(ValueError, match="at most 2\\^20 samples"):  # (every slot's bound)
        plan(sc.program((1 << 20) + 2))
    assert (_lib.SPECTRUM_F32_POW2_MAX, _lib.SPECTRUM_F32_ANY_MAX) == (sc.F32_POW2_MAX, sc.F32_ANY_MAX) == (16384, 4096)


def test_any_other_program_with_either_op_is_refused_by_name():
    shape = "DSP_OP_PSD / DSP_OP_FFT \\(psd, fft\\) run on dsp_spectrum_kernel only, on rows in memory: the program must be exactly LOAD, PSD, STORE or LOAD, FFT, STORE"
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
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=1)  # nothing reads the spectrum in the same program
    with pytest.raises(NotImplementedError, match=shape):
        plan(p)
    for rows, loop in ((np.int32, np.float64), (np.uint32, np.float64)):
        with pytest.raises(NotImplementedError, match="the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(sc.program(1000, "psd", rows, loop), loop)
    p = sc.program(1000, loop=np.float64)  # float32 loop, float64 output
    with pytest.raises((NotImplementedError, ValueError)):
        plan(p)
    p = sc.program(1000)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # the spectrum into the row's own slot
    with pytest.raises(ValueError, match="bad PSD"):
        plan(p)


def test_the_opcodes_are_appended_and_the_registry_lists_the_two_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _PROCESSOR_FILES, module_accepted

    assert (_lib.OP_TIME_OVER_THRESHOLD, _lib.OP_PSD, _lib.OP_FFT) == (38, 39, 40)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_PSD 39" in header and "#define DSP_OP_FFT 40" in header and "#define DSP_OP_TIME_OVER_THRESHOLD 38" in header
    assert processors.SPECTRAL == ("fft", "psd") and not set(processors.SPECTRAL) & set(processors.__all__) and not set(processors.SPECTRAL) & set(_PROCESSOR_FILES)
    g = processors.psd
    assert g.signature == "(n),(m)" and g.types == ["ff", "dd"] and (g.nin, g.nout) == (2, 0) and g.__name__ == "psd"
    g = processors.fft
    assert g.signature == "(n),(m)" and g.types == ["fF", "dD"] and (g.nin, g.nout) == (2, 0) and g.__name__ == "fft"
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "dsp_psd") and hasattr(L, "dsp_fft") and {"dsp_psd", "dsp_fft"} <= set(_lib.EXPORTS)
    for name in processors.SPECTRAL:
        assert module_accepted(M, name) and module_accepted(f"{M}.fft", name) and module_accepted("dspeed_amd.processors", name)
        assert not module_accepted(f"{M}.histogram", name)
    assert not module_accepted(f"{M}.fft", "histogram") and not hasattr(processors, "ifft")


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the two entries that name their loop in an argument instead of a suffix"""

    def _entry(self, name, args):
        self.calls.append([name] + [self._name(a) for a in args])
        return 0

    def dsp_psd(self, *args):
        return self._entry("dsp_psd", args)

    def dsp_fft(self, *args):
        return self._entry("dsp_fft", args)


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
ROW_KINDS = {"1d-f32": ((LEN,), np.float32), "f32": ((N_WF, LEN), np.float32), "i16": ((N_WF, LEN), np.int16), "u16": ((N_WF, LEN), np.uint16),
             "f64": ((N_WF, LEN), np.float64), "i32": ((N_WF, LEN), np.int32), "f32-17": ((N_WF, 17), np.float32), "f32-long": ((1, 4097), np.float32)}


def _cases():
    out = []
    for name in ("psd", "fft"):
        for rows in ROW_KINDS:
            out.append((name, rows, "passed", ()))
        out += [(name, "f32", "omitted", ()), (name, "f32", "none", ()), (name, "f32", "wrong-shape", ()), (name, "f32", "wrong-type", ()),
                (name, "f32", "passed", ("rows", "out")), (name, "f64", "passed", ("rows",)), (name, "i16", "passed", ("out",))]
    return out


CASES = _cases()


def case_id(case):
    name, rows, outs, device = case
    return "-".join([name, rows, f"outs:{outs}"] + [f"dev:{d}" for d in device])


def record(case):
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    name, rows, outs, device = case
    made = []
    with _installed() as fake:
        try:
            shape, dtype = ROW_KINDS[rows]
            w = (np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)
            loop = np.float32 if dtype in (np.float32, np.int16, np.uint16) else np.float64
            ot = loop if name == "psd" else (np.complex64 if loop is np.float32 else np.complex128)
            if outs == "wrong-type":
                ot = np.float64 if name == "psd" else np.complex128
            m = shape[-1] // 2 + 1 + (1 if outs == "wrong-shape" else 0)
            o = np.zeros(shape[:-1] + (m,), dtype=ot)
            if "rows" in device:
                made.append(DeviceArray.from_numpy(w))
                w = made[-1]
            if "out" in device:
                made.append(DeviceArray.from_numpy(o))
                o = made[-1]
            args = {"passed": (w, o), "wrong-shape": (w, o), "wrong-type": (w, o), "omitted": (w,), "none": (w, None)}[outs]
            try:
                r = getattr(processors, name)(*args)
                result = {"result": [type(r).__name__, str(r.dtype), list(r.shape), r is o]}
            except Exception as e:  # noqa: BLE001 -- (type and text are what is recorded)
                result = {"raises": [type(e).__name__, str(e)]}
            result["calls"] = fake.calls
            result["live"] = fake.live() - len(made)
        finally:
            for d in made:
                d.free()
    return json.loads(json.dumps(result))


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def test_calls_are_the_recorded_ones(golden):
    assert sorted(golden) == sorted(case_id(c) for c in CASES) and len(golden) == len(CASES)
    for case in CASES:
        got = record(case)
        assert got == golden[case_id(case)], case_id(case)
        assert got["live"] == 0, case_id(case)  # (whatever the call raised)


def test_what_the_records_say(golden):
    """one entry for both loops: the loop's type is the sixth argument; fft's rows are 2 m values of it apart"""
    call = golden["psd-f32-outs:passed"]["calls"]
    assert len(call) == 1 and call[0][0] == "dsp_psd" and call[0][2:6] == [_lib.F32, N_WF, LEN, LEN] and call[0][6] == _lib.F32 and call[0][8:10] == [9, 9]
    call = golden["fft-f64-outs:passed"]["calls"][0]
    assert call[0] == "dsp_fft" and call[2:6] == [_lib.F64, N_WF, LEN, LEN] and call[6] == _lib.F64 and call[8:10] == [9, 18]
    assert golden["fft-i16-outs:passed"]["calls"][0][2] == _lib.I16 and golden["psd-u16-outs:passed"]["calls"][0][2] == _lib.U16
    assert golden["psd-1d-f32-outs:passed"]["result"] == ["ndarray", "float32", [9], True]
    assert golden["fft-f32-outs:passed-dev:rows-dev:out"]["result"] == ["DeviceArray", "complex64", [N_WF, 9], True]
    for name in ("psd", "fft"):
        must = f"{name}(w_in, {name}_out): {name}_out must be passed (len(w_in)//2 + 1 bins)"
        assert golden[f"{name}-f32-outs:omitted"]["raises"] == ["TypeError", must] and golden[f"{name}-f32-outs:none"]["raises"] == ["TypeError", must]
        assert golden[f"{name}-f32-outs:wrong-shape"]["raises"][0] == "DSPFatal"
        assert golden[f"{name}-f32-outs:wrong-shape"]["raises"][1].startswith(f"Size of {name} must be len(w_in)//2+1 = 9")
        assert golden[f"{name}-i32-outs:passed"]["raises"] == ["NotImplementedError", f"{name}: the float64 loop takes float64 rows on the device"]
        assert golden[f"{name}-f32-long-outs:passed"]["raises"] == ["NotImplementedError", f"{name}: {LIMITS} (4097 given): a row's transform lives in 64 KiB of LDS"]
        assert golden[f"{name}-f32-outs:wrong-type"]["raises"][0] == "TypeError"
        for k in golden:
            if "raises" in golden[k]:
                assert golden[k]["calls"] == []


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


DECLARED = "psd_out(len({0})//2+1, period=1/{0}.period/len({0}))"


def _recipe(source="waveform", first=None):
    procs = dict(first or {})
    name = source.split("[")[0]
    procs["psd_out"] = {"function": "psd", "module": f"{M}.fft", "args": [source, DECLARED.format(name) if "[" not in source else "psd_out(1501)"]}
    procs["p_max"] = {"function": "amax", "module": "numpy", "args": ["psd_out[1:]", 1, "p_max"], "kwargs": {"signature": "(n),()->()", "types": ["fi->f"]}}
    return procs


def _table(n=4096, rows=12):
    from dspeed_amd.processing_chain import WaveformInput

    rng = np.random.default_rng(7)
    return {"waveform": WaveformInput((10000 + rng.integers(-20, 21, (rows, n))).astype(np.uint16), 16.0), "bl": rng.uniform(9990, 10010, rows).astype(np.float32)}


def test_the_reference_s_declaration_builds_and_keeps_its_period():
    from dspeed_amd.language import Frequency, FrequencyGrid, Grid, _Builder
    from dspeed_amd.processing_chain import build_processing_chain

    tb = _table()
    chain, _, out = build_processing_chain({"outputs": ["psd_out", "p_max"], "processors": _recipe()}, tb)
    stages = _stages(chain)
    assert stages == [("psd psd_out on rows", KERNEL, [_lib.OP_LOAD, _lib.OP_PSD, _lib.OP_STORE])]  # (the rows are a chain input: nothing written first)
    assert out["psd_out"].shape == (12, 2049) and out["psd_out"].dtype == np.float32 and out["p_max"].shape == (12,)
    b = _Builder(tb, None)
    v = b.eval_arg(DECLARED.format("waveform"), ["psd_out"])
    assert v.length == 2049 and isinstance(v.grid, FrequencyGrid) and v.grid.period == 1 / 16.0 / 4096 and v.grid.offset == 0
    assert v.grid != Grid(v.grid.period) and v.grid.shifted(1).offset == v.grid.period and isinstance(v.grid.shifted(1), FrequencyGrid)
    q = b.eval_arg("q(5, period=psd_out.period*2, offset=3)", ["q"])  # (a spectrum's period read back: a frequency again; an offset in bins)
    assert isinstance(q.grid, FrequencyGrid) and q.grid.period == 2 * v.grid.period and q.grid.offset == 3 * q.grid.period
    for text in ("1/waveform.period", "psd_out.period*2"):  # a frequency lives in a declaration's period= / offset= only
        with pytest.raises(ProcessingChainError, match="number / time is not supported"):
            b.eval_arg(text)
    with pytest.raises(ProcessingChainError, match="scaled by plain numbers only"):
        b.eval_arg("r(5, period=1/waveform.period + 1)", ["r"])
    assert isinstance(Frequency(2.0) * 1, float)


def test_sources_a_slice_and_a_waveform_the_program_computes():
    from dspeed_amd.processing_chain import build_processing_chain

    blsub = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]}}
    chain, _, out = build_processing_chain({"outputs": ["psd_out", "p_max"], "processors": _recipe("wf_blsub", blsub)}, _table())
    stages = _stages(chain)
    whats = [s[0] for s in stages]
    assert whats.index("wf_blsub -> HBM") < whats.index("psd psd_out on rows") and [s[1] for s in stages].count(KERNEL) == 1
    chain, _, out = build_processing_chain({"outputs": ["psd_out", "p_max"], "processors": _recipe("wf_blsub[:3000]", blsub)}, _table())
    stages = _stages(chain)
    mine = next(s for s in stages if s[1] == KERNEL)
    assert mine[2] == [_lib.OP_LOAD, _lib.OP_PSD, _lib.OP_STORE] and out["psd_out"].shape == (12, 1501)
    io = next(st["program"].io for st in chain._stages if st["what"] == mine[0])
    assert [(i[3], i[4]) for i in io if i[1] == _lib.IO_WF_IN] == [(3000, 0)]
    chain, _, out = build_processing_chain({"outputs": ["psd_out"], "processors": _recipe("waveform[96:3096]")}, _table())
    io = chain._stages[0]["program"].io
    assert [(i[3], i[4]) for i in io if i[1] == _lib.IO_WF_IN] == [(3000, 96)] and not any("-> HBM" in s[0] for s in _stages(chain))


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import build_processing_chain

    def build(procs, table=None, outputs=("psd_out",)):
        return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table())

    def one(fn, args, module=M):
        return {"psd_out": {"function": fn, "module": module, "args": args}}

    with pytest.raises(DSPFatal, match="Size of psd must be len\\(w_in\\)//2\\+1 = 2049"):
        build(one("psd", ["waveform", "psd_out(2048)"]))
    with pytest.raises(ProcessingChainError, match="declare the output as name\\(len\\(w_in\\)//2\\+1\\): 2049 bins"):
        build(one("psd", ["waveform", "psd_out"]))
    with pytest.raises(NotImplementedError, match="processor 'fft' \\(psd_out\\): complex variables are not in the recipe language"):
        build(one("fft", ["waveform", "psd_out(2049)"], f"{M}.fft"))
    with pytest.raises(NotImplementedError, match="processor 'ifft' is not implemented on the device path"):
        build(one("ifft", ["waveform", "psd_out(2049)"]))
    with pytest.raises(NotImplementedError, match=f"psd \\(psd_out\\): {LIMITS} \\(5000 given\\)"):
        build(one("psd", ["waveform", "psd_out(2501)"]), _table(5000))
    tb64 = {"waveform": _table()["waveform"].values.astype(np.float64)}
    with pytest.raises(NotImplementedError, match="psd in a recipe whose loop type is float64"):
        build(one("psd", ["waveform", "psd_out(2049)"]), tb64)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="psd.*DSPEED_HIP_NO_STAGES"):
        build(one("psd", ["waveform", "psd_out(2049)"]))
