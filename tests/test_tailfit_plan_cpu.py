"""The planner's, the registry's and the recipe compiler's part of the decay-tail fitter without a device (dsp_chain_plan): DSP_OP_LOG_CHECK,
DSP_OP_POLY_FIT, DSP_OP_POLY_DIFF and DSP_OP_POLY_EXP_RMS have one route -- dsp_tailfit_kernel, whatever the switches say --, their program
shapes (each with or without a BL_SUBTRACT behind the LOAD) and every refusal by name; the opcodes are appended; the four processors are
attributes of the registry listed in ``TAILFIT``; what a call hands to the library (against a subclass of tests/fake_dsp_lib.FakeLib);
``init_args``; the stages of the recipe bl_subtract -> log_check -> poly_fit -> poly_diff | poly_exp_rms."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import fake_dsp_lib
import tailfit_cases as tc
from dspeed_amd import _lib
from dspeed_amd.chain import plan
from dspeed_amd.errors import ProcessingChainError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = tc.KERNEL
F64 = dict(rows=np.float64, loop=np.float64)
L, BL, LG, PF, PD, PE, ST, SS = (_lib.OP_LOAD, _lib.OP_BL_SUBTRACT, _lib.OP_LOG_CHECK, _lib.OP_POLY_FIT, _lib.OP_POLY_DIFF, _lib.OP_POLY_EXP_RMS, _lib.OP_STORE,
                                 _lib.OP_STORE_SCALAR)
NAMES = ("DSP_OP_LOG_CHECK / DSP_OP_POLY_FIT / DSP_OP_POLY_DIFF / DSP_OP_POLY_EXP_RMS \\(log_check, poly_fit, poly_diff, poly_exp_rms\\) run on dsp_tailfit_kernel only, "
         "on rows in memory: ")
SHAPES = NAMES + "the program must be exactly LOAD, LOG_CHECK, STORE; or LOAD, POLY_FIT, STORE; or LOAD, LOAD of the coefficients, POLY_DIFF \\| POLY_EXP_RMS, STORE_SCALAR, STORE_SCALAR"

# every shape the kernel runs: what tc.program takes, and the ops it must give
EVERY_SHAPE = [
    (dict(log=True), [L, LG, ST]),
    (dict(fit=True), [L, PF, ST]),
    (dict(resid="diff"), [L, L, PD, SS, SS]),
    (dict(resid="exp"), [L, L, PE, SS, SS]),
    (dict(log=True, fit=True), [L, LG, PF, ST, ST]),
    (dict(log=True, fit=True, store_log=False), [L, LG, PF, ST]),
    (dict(fit=True, resid="diff"), [L, PF, PD, ST, SS, SS]),
    (dict(fit=True, resid="exp", store_pars=False), [L, PF, PE, SS, SS]),
    (dict(log=True, fit=True, resid="diff", resid_of="log"), [L, LG, PF, PD, ST, ST, SS, SS]),
    (dict(log=True, fit=True, resid="exp", store_log=False), [L, LG, PF, PE, ST, SS, SS]),
    (dict(log=True, fit=True, resid="exp", store_pars=False), [L, LG, PF, PE, ST, SS, SS]),
    (dict(log=True, fit=True, resid="diff", resid_of="log", store_log=False, store_pars=False), [L, LG, PF, PD, SS, SS]),
]


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_every_shape_takes_the_tailfit_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for kw, ops in EVERY_SHAPE:
            assert [op[0] for op in tc.program(129, **kw).ops] == ops
            for n in tc.LENGTHS + (8192,):
                m = 4 if n < 8192 else 2
                assert plan(tc.program(n, m=m, **kw))["kernel"] == KERNEL, (kw, n)
                assert plan(tc.program(n, m=m, **kw, **F64), np.float64)["kernel"] == KERNEL
            with_sub = [op[0] for op in tc.program(129, subtract=1000.0, **kw).ops]
            assert BL in with_sub and [o for o in with_sub if o != BL] == ops
            assert plan(tc.program(129, subtract="column", **kw))["kernel"] == KERNEL and plan(tc.program(129, subtract=1000.0, **kw))["kernel"] == KERNEL
            for rows in (np.int16, np.uint16):
                assert plan(tc.program(1000, rows, offset=3, row_stride=1007, out_stride=1005, **kw))["kernel"] == KERNEL
        for m in tc.MS:
            assert plan(tc.program(65, fit=True, m=m))["kernel"] == KERNEL and plan(tc.program(65, resid="exp", m=m, pars_stride=m + 3))["kernel"] == KERNEL
        # the BL_SUBTRACT and the LOAD of the coefficients in either order
        p = tc.program(129, resid="diff", subtract=3.0)
        assert [op[0] for op in p.ops] == [L, L, BL, PD, SS, SS]
        p.ops[1], p.ops[2] = p.ops[2], p.ops[1]
        assert plan(p)["kernel"] == KERNEL

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_geometry_the_case_book_assumes_is_the_headers():
    kernels_h = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    mine = kernels_h[kernels_h.index("namespace dsp_tailfit {"):kernels_h.index("}  // namespace dsp_tailfit")]
    assert "using dsp_pileup::TS;" in mine and "using dsp_pileup::ROWS;" in mine and "constexpr int POLY_MAX = 8;" in mine
    assert "constexpr int ROWS = 64, TS = 64, PITCH = TS + 1;" in kernels_h
    assert {63, 64, 65, 129} <= set(tc.LENGTHS) and {63, 64, 65, 130} <= set(tc.ROW_COUNTS) and min(tc.LENGTHS) == 1 and max(tc.MS) == _lib.POLY_MAX == 8
    program_h = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_program.h")).read()
    assert "#define DSP_POLY_MAX 8" in program_h
    g = plan(tc.program(1000, log=True, fit=True, resid="exp"))
    assert g["kernel"] == KERNEL


def test_any_other_program_with_the_ops_is_refused_by_name():
    p = tc.program(1000, log=True)
    p.ops.pop()  # the logarithm, nothing stored
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = tc.program(1000, fit=True)
    p.ops.pop()  # the fit, nothing stored
    with pytest.raises(NotImplementedError, match=NAMES):
        plan(p)
    p = tc.program(1000, log=True)
    p.ops.insert(1, (_lib.OP_POLE_ZERO, 0, 0, 0, (), (__import__("dspeed_amd.chain", fromlist=["Scalar"]).Scalar.const(100.0),)))  # an intermediate as the source
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = tc.program(1000, log=True, fit=True)
    p.ops.insert(2, p.ops[1])  # two logarithms
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = tc.program(1000, log=True, fit=True, resid="exp")
    p.ops.pop()  # rms not stored
    with pytest.raises(NotImplementedError, match=NAMES + "the program must be exactly"):
        plan(p)
    p = tc.program(1000, log=True, resid="diff")  # the residuals of a logarithm against coefficients from memory: not a shape
    with pytest.raises(NotImplementedError, match=SHAPES):
        plan(p)
    p = tc.program(1000, log=True, fit=True)
    p.ops[2] = p.ops[2][:2] + (0,) + p.ops[2][3:]  # the fit of the raw row beside a logarithm
    with pytest.raises(NotImplementedError, match=NAMES + "poly_fit in the same program reads exactly the logged row; the residuals the row as loaded or the logged row, with exactly the fitted coefficients"):
        plan(p)
    p = tc.program(1000, log=True, fit=True)
    p.ops[4] = p.ops[3]  # the logged row stored twice, the coefficients never
    with pytest.raises(NotImplementedError, match=NAMES + "the logged row and the coefficients are stored once each, whole, in the loop's type; the two results of the residuals once each"):
        plan(p)
    p = tc.program(1000, resid="diff")
    p.ops[-1] = p.ops[-2]  # mean stored twice
    with pytest.raises(NotImplementedError, match=NAMES + "the logged row and the coefficients are stored once each"):
        plan(p)
    p = tc.program(1000, resid="exp")
    p.io[1] = p.io[1][:2] + (_lib.I16,) + p.io[1][3:]  # coefficients of another type than the loop's
    with pytest.raises(NotImplementedError, match=NAMES + "the coefficients are loaded whole into slot ip\\[0\\], a row of them per event in the loop's type"):
        plan(p)
    p = tc.program(1000, log=True, subtract=1.0)
    p.ops[1] = p.ops[1][:4] + ((1,),) + p.ops[1][5:]  # numpy.subtract keeps NaN samples single: not the subtraction that is folded in
    with pytest.raises(NotImplementedError, match=NAMES + "the BL_SUBTRACT behind the LOAD works on the rows in place \\(bl_subtract, ip\\[0\\] = 0\\)"):
        plan(p)
    for rows in (np.int32, np.uint32):
        with pytest.raises(NotImplementedError, match=NAMES + "the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(tc.program(1000, rows, np.float64, log=True), np.float64)
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(tc.program(1000, np.float64, np.float32, log=True))


def test_the_planners_argument_errors_and_limits():
    with pytest.raises(ValueError, match="log_check: the output has the length of the input \\(len\\(w_in\\) = 1000, len\\(w_log\\) = 999\\)"):
        plan(tc.program(1000, log=True, out_len=999))
    for kw in (dict(fit=True), dict(resid="diff"), dict(resid="exp"), dict(log=True, fit=True, resid="exp")):
        name = "poly_fit" if "fit" in kw else ("poly_diff" if kw["resid"] == "diff" else "poly_exp_rms")
        with pytest.raises(NotImplementedError, match=f"{name}: at most 8 coefficients \\(9 given\\): a lane keeps one float64 accumulator each"):
            plan(tc.program(1000, m=9, **kw))
        assert plan(tc.program(512, m=8, **kw))["kernel"] == KERNEL  # 511**7 < 2**63
        with pytest.raises(NotImplementedError, match=f"{name}: \\(n - 1\\)\\*\\*\\(m - 1\\) must stay below 2\\*\\*63 \\(n = 514 samples, m = 8 coefficients\\): beyond it the "
                                                      "reference's int64 power i\\*\\*j wraps silently"):
            plan(tc.program(514, m=8, **kw))  # 513**7 > 2**63
        assert plan(tc.program(1 << 20, m=4, **kw))["kernel"] == KERNEL and plan(tc.program(1 << 20, m=1, **kw))["kernel"] == KERNEL
    assert 511**7 < 2**63 < 513**7
    with pytest.raises(ValueError, match="poly_fit: io is a DSP_IO_TAPS binding of m \\* m = 16 DSP_F64 values, the inverted matrix of power sums \\(both loops\\)"):
        plan(tc.program(1000, fit=True, inv_len=15))
    with pytest.raises(ValueError):  # float32 taps in the float64 loop: no program's
        plan(tc.program(1000, fit=True, inv_dtype=np.float32, **F64), np.float64)
    with pytest.raises(ValueError, match="poly_fit: io is a DSP_IO_TAPS binding of m \\* m = 16 DSP_F64 values"):
        plan(tc.program(1000, fit=True, inv_dtype=np.float32))
    p = tc.program(1000, log=True)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # destination = source
    with pytest.raises(ValueError, match="bad LOG_CHECK \\(src: the slot of the row; dst: another slot, for the logged row\\)"):
        plan(p)
    p = tc.program(1000, fit=True)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]
    with pytest.raises(ValueError, match="bad POLY_FIT \\(src: the slot of the row; dst: another slot, for the coefficients; io: the inverted matrix\\)"):
        plan(p)
    p = tc.program(1000, resid="diff")
    p.n_sregs = 1  # no register for rms
    with pytest.raises(ValueError, match="bad POLY_DIFF \\(src: the slot of the row; ip\\[0\\]: the slot of the coefficients; dst, dst \\+ 1: the registers of mean and rms\\)"):
        plan(p)


def test_the_opcodes_are_appended_and_the_registry_lists_the_processors_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _PROCESSOR_FILES, _SIGS, _TAILFIT_FILES, module_accepted

    assert (_lib.OP_MULTI_A_FILTER, _lib.OP_LOG_CHECK, _lib.OP_POLY_FIT, _lib.OP_POLY_DIFF, _lib.OP_POLY_EXP_RMS) == (49, 50, 51, 52, 53)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    for line in ("#define DSP_OP_LOG_CHECK 50", "#define DSP_OP_POLY_FIT 51", "#define DSP_OP_POLY_DIFF 52", "#define DSP_OP_POLY_EXP_RMS 53"):
        assert line in header
    assert processors.TAILFIT == ("log_check", "poly_fit", "poly_diff", "poly_exp_rms")
    others = (set(processors.__all__) | set(processors.SPECTRAL) | set(processors.ORDER) | set(processors.RESAMPLING) | set(processors.ML)
              | set(processors.SMOOTHING) | set(processors.PILEUP) | set(processors.PULSES) | set(_PROCESSOR_FILES))
    assert not set(processors.TAILFIT) & others
    g = processors.log_check
    assert g.signature == "(n)->(n)" and g.types == ["f->f", "d->d"] and g.nargs == 2 and g.__name__ == "log_check"
    for g in (processors.poly_diff, processors.poly_exp_rms):
        assert g.signature == "(n),(m)->(),()" and g.types == ["ff->ff", "dd->dd"] and g.nargs == 4
    assert callable(processors.poly_fit) and not hasattr(processors.poly_fit, "signature")  # a factory, as in the reference
    g = processors.poly_fit(100, 3)
    assert g.__name__ == "poly_fitter" and g.signature == "(n),(m)" and g.types == ["ff", "dd"] and g.nin == 2 and g.nout == 0 and g.__doc__ == "Fit w_in to order 3 polynomial."
    assert g.inv.shape == (4, 4) and g.inv.dtype == np.float64 and np.array_equal(g.inv, tc.inverse(100, 3))
    assert _SIGS["log_check"] == "wW" and _SIGS["poly_fit"] == "wW" and _SIGS["poly_diff"] == _SIGS["poly_exp_rms"] == "wwSS"
    assert _TAILFIT_FILES == {"log_check": ("log_check",), "poly_fit": ("poly_fit",), "poly_diff": ("poly_fit",), "poly_exp_rms": ("poly_fit",)}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for entry in ("dsp_log_check_rows", "dsp_poly_fit_rows", "dsp_poly_residual_rows"):
        assert hasattr(lib, entry) and entry in _lib.EXPORTS
    for fn, file in _TAILFIT_FILES.items():
        assert module_accepted(M, fn) and module_accepted("dspeed_amd.processors", fn) and module_accepted(f"{M}.{file[0]}", fn) and not module_accepted(f"{M}.rc_cr2", fn)
    assert not module_accepted(f"{M}.poly_fit", "log_check") and not module_accepted(f"{M}.log_check", "poly_diff")


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entries that name their loop in an argument instead of a suffix"""

    def _record(self, name, args):
        self.calls.append([name] + [self._name(a) for a in args])
        return 0

    def dsp_log_check_rows(self, *args):
        return self._record("dsp_log_check_rows", args)

    def dsp_poly_fit_rows(self, *args):
        return self._record("dsp_poly_fit_rows", args)

    def dsp_poly_residual_rows(self, *args):
        return self._record("dsp_poly_residual_rows", args)


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
    """rows (pointer, type, count, length, stride), the loop's type, then: the output and its stride; the matrix, m, the coefficients and their
    stride; which residual, the coefficients, m, their stride, mean, rms; the stream, the row of an error"""
    from dspeed_amd import processors

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    with _installed() as fake:
        r = processors.log_check(_rows(dtype))  # the output left out: a new array of the loop's type
        assert isinstance(r, np.ndarray) and r.shape == (N_WF, LEN) and r.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_log_check_rows" and len(call) == 11
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == ["ptr", 1, 0, N_WF * LEN * esz] and call[8] == LEN and call[9] is None and call[10] == "byref"
        assert fake.live() == 0
        del fake.calls[:]
        pars = np.zeros((N_WF, 3), loop)
        assert processors.poly_fit(LEN, 2)(_rows(dtype), pars) is pars
        (call,) = fake.calls
        assert call[0] == "dsp_poly_fit_rows" and len(call) == 13 and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        k = call[1][1]  # (allocations count on from call to call)
        assert call[7] == ["ptr", k + 1, 0, 9 * 8] and call[8] == 3 and call[9] == ["ptr", k + 2, 0, N_WF * 3 * esz] and call[10] == 3 and call[11] is None and call[12] == "byref"
        assert fake.live() == 0
        del fake.calls[:]
        for exp_rms, g in ((0, processors.poly_diff), (1, processors.poly_exp_rms)):
            mean, rms = g(_rows(dtype), np.array([1.0, 0.5]))  # one row of coefficients for every event: repeated on the way to the device
            assert mean.shape == rms.shape == (N_WF,) and mean.dtype == rms.dtype == loop
            (call,) = fake.calls
            assert call[0] == "dsp_poly_residual_rows" and len(call) == 15 and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code and call[7] == exp_rms
            k = call[1][1]
            assert call[8] == ["ptr", k + 1, 0, N_WF * 2 * esz] and call[9:11] == [2, 2] and call[11] == ["ptr", k + 2, 0, N_WF * esz] and call[12] == ["ptr", k + 3, 0, N_WF * esz]
            assert call[13] is None and call[14] == "byref" and fake.live() == 0
            del fake.calls[:]
        mean, rms = processors.poly_diff(_rows(dtype, (LEN,)), np.zeros(4, loop))  # a 1-D call: two values
        assert np.ndim(mean) == 0 and np.ndim(rms) == 0 and fake.calls[0][2:6] == [code, 1, LEN, LEN] and fake.calls[0][9:11] == [4, 4]


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors

    w = _rows(np.float32)
    with _installed() as fake:
        for g, args in ((processors.log_check, ()), (processors.poly_diff, (np.zeros(2),)), (processors.poly_fit(LEN, 1), ())):
            with pytest.raises(NotImplementedError, match="the float64 loop takes float64 rows on the device$"):
                g(_rows(np.int32), *args)
        with pytest.raises(ValueError, match="^log_check: the output has the length of the input \\(len\\(w_in\\) = 16, len\\(w_log\\) = 17\\)$"):
            processors.log_check(w, np.zeros((N_WF, LEN + 1), np.float32))
        with pytest.raises(TypeError, match="takes 1 inputs and 1 outputs"):
            processors.log_check(w, w, w)
        for g in (processors.poly_diff, processors.poly_exp_rms):
            with pytest.raises(NotImplementedError, match=f"^{g.__name__}: at most 8 coefficients \\(9 given\\): a lane keeps one float64 accumulator each$"):
                g(w, np.zeros(9))
            with pytest.raises(ValueError, match=f"^{g.__name__}: at least one coefficient$"):
                g(w, np.zeros((N_WF, 0)))
            with pytest.raises(ValueError, match="poly_pars has shape \\(2, 4\\), expected \\(3, m\\) or \\(m,\\)"):
                g(w, np.zeros((2, 4)))
        with pytest.raises(NotImplementedError, match="^poly_diff: \\(n - 1\\)\\*\\*\\(m - 1\\) must stay below 2\\*\\*63 \\(n = 514 samples, m = 8 coefficients\\): beyond it the reference's "
                                                      "int64 power i\\*\\*j wraps silently$"):
            processors.poly_diff(np.ones((2, 514), np.float32), np.zeros(8))
        with pytest.raises(ValueError, match="^poly_fitter: poly_pars holds deg \\+ 1 = 2 coefficients \\(3 given\\)$"):
            processors.poly_fit(LEN, 1)(w, np.zeros((N_WF, 3), np.float32))
        with pytest.raises(NotImplementedError, match="^poly_fit: at most 8 coefficients \\(9 given\\)"):
            processors.poly_fit(100, 8)
        for bad in (-1, 2.5):
            with pytest.raises(ValueError, match="poly_fit: (length|deg) is a non-negative integer"):
                processors.poly_fit(100, bad)
            with pytest.raises(ValueError, match="poly_fit: (length|deg) is a non-negative integer"):
                processors.poly_fit(bad, 1)
        with pytest.raises(NotImplementedError, match="^poly_fit: length is a constant of the call on the device, not a per-event value$"):
            processors.poly_fit(np.array([100, 101]), 1)
        with pytest.raises(np.linalg.LinAlgError):  # length <= deg: the factory's matrix is singular, as in the reference
            processors.poly_fit(2, 3)
        assert fake.calls == [] and fake.live() == 0


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _table(rows=None, n_rows=24, n=1000):
    from dspeed_amd.processing_chain import WaveformInput

    w = (1000 + (np.arange(n_rows * n).reshape(n_rows, n) * 7) % 41).astype(np.uint16) if rows is None else rows
    return {"waveform": WaveformInput(w, 16.0), "bl": np.full(len(w), 900, np.float32), "deg": np.full(len(w), 3, np.int32)}


RES = "tail_mean, tail_rms"


def _recipe(source="wf_blsub", resid="poly_exp_rms", resid_of=None, init=("len(wf_logged)", 3), pars="fit_pars(shape=4)", module=M, fit_function=f"{M}.poly_fit"):
    fit = {"function": fit_function, "args": ["wf_logged", pars], "init_args": list(init)}
    if "." not in fit_function:
        fit["module"] = module
    return {
        "wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]},
        "wf_logged": {"function": "log_check", "module": module if module == M else f"{M}.log_check", "args": [source, "wf_logged"]},
        "fit_pars": fit,
        RES: {"function": resid, "module": module if module == M else f"{M}.poly_fit", "args": [resid_of or source, "fit_pars", "tail_mean", "tail_rms"]},
    }


def _build(procs, outputs, table=None, db=None):
    from dspeed_amd.processing_chain import build_processing_chain

    return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table(), db_dict=db)


def test_the_docstring_chain_is_one_launch_with_the_subtraction_folded_in():
    for kw in ({}, dict(module=f"{M}.files"), dict(fit_function="poly_fit")):  # the package's string, the files' strings, the plain name
        chain, _, out = _build(_recipe(**kw), ["fit_pars", "tail_mean", "tail_rms"])
        mine = [s for s in _stages(chain) if s[1] == KERNEL]
        assert mine == [(f"log_check wf_logged + poly_fit fit_pars + poly_exp_rms {RES} in one launch on rows", KERNEL, [L, BL, LG, PF, PE, ST, SS, SS])]
        stage = next(st for st in chain._stages if st["what"] == mine[0][0])
        assert [o[0] for o in stage["outs"]] == ["out:fit_pars", "out:tail_mean", "out:tail_rms"]  # no logged row, no subtracted row
        assert stage["program"].ops[1][5][0].kind == _lib.ARG_INPUT  # the baseline: the table's column
        (inv,) = [v for k, v in stage["consts"].items() if k.startswith("taps:inv#")]
        assert inv.dtype == np.float64 and np.array_equal(inv.reshape(4, 4), tc.inverse(1000, 3))  # len(wf_logged) = 1000
        assert [(i[1], i[3]) for i in stage["program"].io if i[1] == _lib.IO_TAPS] == [(_lib.IO_TAPS, 16)]
        assert not any(op[0] in (BL, LG, PF, PD, PE) for op in chain._program.ops)
        assert out["fit_pars"].shape == (24, 4) and out["fit_pars"].dtype == np.float32 and out["tail_mean"].shape == out["tail_rms"].shape == (24,)
    # poly_diff of the logged row: the same launch
    chain, _, out = _build(_recipe(resid="poly_diff", resid_of="wf_logged"), ["tail_rms"])
    assert [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, BL, LG, PF, PD, SS, SS]]


def test_with_a_slice_the_subtracted_rows_are_written_first_and_read_at_their_start():
    chain, _, out = _build(_recipe(source="wf_blsub[700:]"), ["fit_pars", "tail_mean", "tail_rms"])
    whats = [s[0] for s in _stages(chain)]
    one = f"log_check wf_logged + poly_fit fit_pars + poly_exp_rms {RES} in one launch on rows"
    assert whats.index("wf_blsub -> HBM") < whats.index(one)
    stage = chain._stages[whats.index(one)]
    assert [op[0] for op in stage["program"].ops] == [L, LG, PF, PE, ST, SS, SS]
    assert [(i[3], i[4]) for i in stage["program"].io if i[1] == _lib.IO_WF_IN] == [(300, 700)]
    (inv,) = [v for k, v in stage["consts"].items() if k.startswith("taps:inv#")]
    assert np.array_equal(inv.reshape(4, 4), tc.inverse(300, 3))  # len(wf_logged) follows the slice
    # a slice of the input itself: nothing to write first
    chain, _, out = _build(_recipe(source="waveform[100:900]"), ["tail_rms", "wf_logged"])
    assert _stages(chain)[0][2] == [L, LG, PF, PE, ST, SS, SS] and out["wf_logged"].shape == (24, 800)


def test_the_logged_row_and_the_coefficients_are_stored_when_asked_for_or_read():
    chain, _, out = _build(_recipe(), ["tail_rms", "wf_logged"])
    assert [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, BL, LG, PF, PE, ST, SS, SS]] and out["wf_logged"].shape == (24, 1000)
    chain, _, out = _build(_recipe(), ["tail_rms", "wf_logged", "fit_pars"])
    assert [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, BL, LG, PF, PE, ST, ST, SS, SS]]
    # both residuals of one fit: the first takes the fit into its launch and stores the coefficients, the second reads them from there
    procs = _recipe(resid="poly_diff", resid_of="wf_logged")
    procs["m2, r2"] = {"function": "poly_exp_rms", "module": M, "args": ["wf_blsub", "fit_pars", "m2", "r2"]}
    chain, _, out = _build(procs, ["tail_rms", "r2"])
    mine = [s[2] for s in _stages(chain) if s[1] == KERNEL]
    assert len(mine) == 2 and [L, L, PE, SS, SS] in mine and any(PF in ops and ops.count(ST) >= 1 for ops in mine)
    # the subtracted waveform asked for: written to memory first, not folded in
    chain, _, out = _build(_recipe(), ["tail_rms", "wf_blsub"])
    assert [s[2] for s in _stages(chain) if s[1] == KERNEL] == [[L, LG, PF, PE, SS, SS]]


def test_one_launch_per_owning_processor():
    procs = _recipe()
    only_log = {k: v for k, v in procs.items() if k in ("wf_blsub", "wf_logged")}
    chain, _, out = _build(only_log, ["wf_logged"])
    assert _stages(chain) == [("log_check wf_logged on rows", KERNEL, [L, BL, LG, ST])]
    log_fit = {k: v for k, v in procs.items() if k != RES}
    chain, _, out = _build(log_fit, ["fit_pars"])
    assert _stages(chain) == [("log_check wf_logged + poly_fit fit_pars in one launch on rows", KERNEL, [L, BL, LG, PF, ST])]
    chain, _, out = _build(log_fit, ["fit_pars", "wf_logged"])
    assert _stages(chain)[0][2] == [L, BL, LG, PF, ST, ST]
    # a fit of rows that are no logarithm; the residuals against coefficients from the table
    fit = dict(procs["fit_pars"], args=["waveform", "fit_pars(shape=4)"], init_args=["len(waveform)", 3])
    chain, _, out = _build({"fit_pars": fit}, ["fit_pars"])
    assert _stages(chain) == [("poly_fit fit_pars on rows", KERNEL, [L, PF, ST])]
    table = dict(_table(), pars=np.zeros((24, 3), np.float32))
    for fn, op in (("poly_diff", PD), ("poly_exp_rms", PE)):
        chain, _, out = _build({RES: {"function": fn, "module": M, "args": ["waveform", "pars", "tail_mean", "tail_rms"]}}, ["tail_mean", "tail_rms"], table)
        assert _stages(chain)[0][1:] == (KERNEL, [L, L, op, SS, SS])


def test_init_args():
    # the accepted forms: numbers, expressions of the language, db values; the coefficients' length from deg + 1 or checked against it
    for init, pars, n_fit, m in ((("len(wf_logged)", 3), "fit_pars(shape=4)", 1000, 4), ((1000, 2), "fit_pars", 1000, 3), (("len(wf_logged) - 200", "1 + 1"), "fit_pars(3)", 800, 3),
                                 (("db.n", "db.deg"), "fit_pars", 500, 2)):
        chain, _, out = _build(_recipe(init=init, pars=pars), ["fit_pars"], db={"n": 500, "deg": 1})
        assert out["fit_pars"].shape == (24, m)
        (inv,) = [v for st in chain._stages for k, v in st["consts"].items() if k.startswith("taps:inv#")]
        assert np.array_equal(inv.reshape(m, m), tc.inverse(n_fit, m - 1))
    with pytest.raises(ProcessingChainError, match="poly_fit \\(fit_pars\\): poly_pars holds deg \\+ 1 = 4 coefficients \\(5 declared\\)"):
        _build(_recipe(pars="fit_pars(shape=5)"), ["fit_pars"])
    with pytest.raises(NotImplementedError, match="poly_fit \\(fit_pars\\): deg is a constant of the call on the device, not a per-event value"):
        _build(_recipe(init=("len(wf_logged)", "deg")), ["fit_pars"])
    with pytest.raises(ProcessingChainError, match="poly_fit \\(fit_pars\\): deg is a non-negative integer"):
        _build(_recipe(init=("len(wf_logged)", 2.5)), ["fit_pars"])
    with pytest.raises(ProcessingChainError, match="poly_fit \\(fit_pars\\): init_args holds length and deg, as the factory takes them"):
        _build(_recipe(init=(1000,)), ["fit_pars"])
    procs = _recipe()
    del procs["fit_pars"]["init_args"]
    with pytest.raises(ProcessingChainError, match="poly_fit \\(fit_pars\\): init_args holds length and deg"):
        _build(procs, ["fit_pars"])
    procs = _recipe()
    procs["wf_logged"]["init_args"] = [3]
    with pytest.raises(NotImplementedError, match="log_check \\(wf_logged\\): init_args builds a processor from a factory; on the device path only poly_fit is one"):
        _build(procs, ["fit_pars"])
    with pytest.raises(NotImplementedError, match="poly_fit \\(fit_pars\\): at most 8 coefficients \\(9 given\\)"):
        _build(_recipe(init=(1000, 8), pars="fit_pars"), ["fit_pars"])
    with pytest.raises(NotImplementedError, match="poly_fit \\(fit_pars\\): \\(n - 1\\)\\*\\*\\(m - 1\\) must stay below 2\\*\\*63 \\(n = 1000 samples, m = 8 coefficients\\)"):
        _build(_recipe(init=(400, 7), pars="fit_pars"), ["fit_pars"])
    with pytest.raises(ProcessingChainError, match="poly_fit \\(fit_pars\\): the matrix of power sums over range\\(2\\) cannot be inverted for deg = 3 \\(Singular matrix\\)"):
        _build(_recipe(init=(2, 3)), ["fit_pars"])


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import WaveformInput

    with pytest.raises(Exception, match="log_check"):
        procs = _recipe()
        procs["wf_logged"]["module"] = f"{M}.poly_fit"  # not log_check's file
        _build(procs, ["tail_rms"])
    with pytest.raises(ProcessingChainError, match="poly_exp_rms \\(tail_mean, tail_rms\\): the coefficients are an array per event"):
        procs = _recipe()
        procs[RES]["args"][1] = "bl"
        _build(procs, ["tail_rms"])
    tb64 = {"waveform": WaveformInput(np.full((4, 100), 1000.0), 16.0), "bl": np.full(4, 900.0)}
    with pytest.raises(NotImplementedError, match="(log_check|poly_fit|poly_exp_rms) in a recipe whose loop type is float64"):
        _build(_recipe(), ["tail_rms"], tb64)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="(log_check|poly_fit|poly_exp_rms) runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        _build(_recipe(), ["tail_rms"])
