"""The planner's, the registry's and the recipe compiler's part of svm_predict without a device (dsp_chain_plan): DSP_OP_SVM_PREDICT has one
route -- dsp_svm_kernel, whatever the switches say --, one program shape and every refusal by name; the opcode is appended; the factory and
its model forms; what a call hands to the library (against a subclass of tests/fake_dsp_lib.FakeLib); the stage list of a cleaning recipe."""
import contextlib
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import fake_dsp_lib
import svm_cases as sc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import ProcessingChainError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = sc.KERNEL
SHAPE = "DSP_OP_SVM_PREDICT \\(svm_predict\\) runs on dsp_svm_kernel only, on rows in memory: the program must be exactly LOAD, SVM_PREDICT, STORE_SCALAR"
LIMIT = "svm_predict: " + sc.LIMITS


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_shape_takes_the_svm_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for n, n_sv, k in ((1, 2, 2), (5, 17, 16), (64, 300, 4), (257, 65, 3), (16384, 3, 23), (256, 2048, 8)):
            assert plan(sc.program(n, n_sv, k))["kernel"] == KERNEL
            assert plan(sc.program(n, n_sv, k, rows=np.float64, loop=np.float64, kind=1, decisions=True), np.float64)["kernel"] == KERNEL
            assert plan(sc.program(n, n_sv, k, loop=np.float64, row_stride=n + 3), np.float64)["kernel"] == KERNEL  # float32 rows, the float64 loop
        assert plan(sc.program(100, 40, 3, decisions=True))["kernel"] == KERNEL  # (float64 decisions beside a float32 label)

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_geometry_and_the_limits_by_name():
    kernels = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    assert "constexpr int CLASSES_MAX = 23, P_MAX = 256, PAIR_BLOCKS_MAX = P_MAX / BLOCK;" in kernels and "constexpr int RESIDENT_MAX = 256;" in kernels
    program = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_program.h")).read()
    assert "#define DSP_SVM_CLASSES_MAX 23" in program and '#define DSP_SVM_LIMITS_TEXT "rows of up to %d samples and models of up to %d classes"' in program
    from dspeed_amd import processors

    assert (_lib.DENSE_N_MAX, _lib.SVM_CLASSES_MAX) == (sc.N_MAX, sc.CLASSES_MAX) and processors.SVM_LIMITS == sc.LIMITS
    for n, k in ((16385, 2), (1 << 19, 3), (10, 24), (16384, 100)):
        for kw, dt in (({}, np.float32), (dict(rows=np.float64, loop=np.float64), np.float64)):
            with pytest.raises(NotImplementedError, match=f"{LIMIT} \\(n = {n}, {k} classes given\\)"):
                plan(sc.program(n, 3, k, **kw), dt)
        with pytest.raises(NotImplementedError, match=f"^svm_predict: {sc.LIMITS} \\(n = {n}, {k} classes given\\)$"):
            processors.check_svm("svm_predict", n, k)
    # the size of a model: a binding's length, in the C entry's words
    assert _lib.SVM_MODEL_MAX == 1 << 28 and "#define DSP_SVM_MODEL_MAX (1 << 28)" in program
    text = re.search(r'#define DSP_SVM_MODEL_TEXT "([^"]*)"', program).group(1)
    processors.check_svm("svm_predict", 16384, 23, 16384), processors.check_svm("svm_predict", 4, 23, (1 << 28) // 253)
    for n, k, n_sv in ((16384, 2, 16385), (4, 23, (1 << 28) // 253 + 1), (4, 2, 0)):
        with pytest.raises(NotImplementedError) as e:
            processors.check_svm("svm_predict", n, k, n_sv)
        assert str(e.value) == "svm_predict: " + text % (1 << 28, n_sv, n, k * (k - 1) // 2)


def test_any_other_program_with_the_op_is_refused_by_name():
    p = sc.program(100, 40, 3)
    p.ops.pop()  # no store
    with pytest.raises(NotImplementedError, match=SHAPE):
        plan(p)
    p = sc.program(100, 40, 3)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=SHAPE):
        plan(p)
    p = sc.program(100, 40, 3)
    p.n_sregs = 2
    p.ops[1] = p.ops[1][:1] + (1,) + p.ops[1][2:]  # the label goes to register 1, register 0 is stored
    with pytest.raises(NotImplementedError, match="DSP_OP_SVM_PREDICT.*the label is stored once, in the loop's type"):
        plan(p)
    for rows in (np.int16, np.uint16):
        with pytest.raises(NotImplementedError, match="DSP_OP_SVM_PREDICT.*the float32 loop takes float32 rows, the float64 loop float32 or float64 rows"):
            plan(sc.program(100, 40, 3, rows=rows))
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(sc.program(100, 40, 3, rows=np.float64))


def test_malformed_operands_are_refused_by_name():
    p = sc.program(100, 40, 3)
    p.ops[1] = p.ops[1][:1] + (5,) + p.ops[1][2:]
    with pytest.raises(ValueError, match="bad SVM_PREDICT \\(src: the slot of the row; dst: the register of the label\\)"):
        plan(p)
    p = sc.program(100, 40, 3)
    p.io[2] = p.io[2][:2] + (_lib.F32,) + p.io[2][3:]  # float32 norms
    with pytest.raises(ValueError, match="svm_predict: support vectors \\(io\\), their squared norms \\(ip\\[0\\]\\), D \\(ip\\[1\\]\\), intercepts \\(ip\\[2\\]\\) and classes \\(ip\\[3\\]\\) are DSP_IO_TAPS bindings of DSP_F64 in both loops"):
        plan(p)
    p = sc.program(100, 40, 3)
    p.io[3] = p.io[3][:3] + (40 * 3 - 1,) + p.io[3][4:]  # D of another shape
    with pytest.raises(ValueError, match="svm_predict: 3 classes, 40 support vectors and rows of 100 samples take 3 intercepts, 4000 support-vector samples and 120 coefficients \\(3, 4000 and 119 given\\)"):
        plan(p)
    p = sc.program(100, 40, 3)
    p.io[5] = p.io[5][:3] + (1,) + p.io[5][4:]  # one class
    with pytest.raises(ValueError, match="svm_predict: a model has at least 2 classes \\(1 given\\)"):
        plan(p)
    p = sc.program(100, 40, 3, kind=2)
    with pytest.raises(ValueError, match="svm_predict: gamma \\(sp\\[0\\]\\), the kernel function \\(sp\\[1\\]: 0 rbf, 1 linear\\) and the decisions' binding \\(sp\\[2\\]\\) are constants of the program"):
        plan(p)
    p = sc.program(100, 40, 3)
    p.ops[1] = p.ops[1][:5] + ((Scalar.const(0.5), Scalar.const(0), Scalar.const(1)),)  # the support vectors as the decisions
    with pytest.raises(ValueError, match="svm_predict: the decisions \\(sp\\[2\\]\\) are a DSP_IO_WF_OUT binding of P = 3 DSP_F64 values a row, or -1"):
        plan(p)


def test_the_opcode_is_appended_and_the_registry_lists_the_processor_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _SIGS, module_accepted

    assert (_lib.OP_WF_CORRECTION, _lib.OP_SVM_PREDICT) == (57, 58)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_SVM_PREDICT 58" in header and not re.search(r"dsp_svm_rows_f(32|64)", header)
    assert processors.CLEANING == ("svm_predict",) and "svm_predict" not in processors.__all__
    assert _SIGS["svm_predict"] == "wS" and module_accepted(M, "svm_predict") and module_accepted(f"{M}.svm", "svm_predict") and not module_accepted(f"{M}.ml", "svm_predict")
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "dsp_svm_rows") and "dsp_svm_rows" in _lib.EXPORTS
    decl = re.search(r"\bint dsp_svm_rows\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == len(_lib.SIG["dsp_svm_rows"]) == 20


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entry that names its loop in an argument instead of a suffix"""

    def dsp_svm_rows(self, *args):
        self.calls.append(["dsp_svm_rows"] + [self._name(a) for a in args])
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


N_WF, LEN, N_SV, K = 3, 16, 9, 4
PAIRS = K * (K - 1) // 2


def _model(kernel="rbf"):
    return sc.synthetic(3, LEN, N_SV, K, kernel, classes=(1, 3, 5, 8))


@pytest.mark.parametrize("dtype, code, loop", [(np.float32, _lib.F32, np.float32), (np.float64, _lib.F64, np.float64)])
def test_the_arguments_of_a_call(dtype, code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, the model's five arrays as bound, their counts, the kernel function and
    gamma, the label, no decisions, the stream, the row of an error"""
    from dspeed_amd import processors as P

    model = _model("linear")
    rows = np.ones((N_WF, LEN), dtype)
    with _installed() as fake:
        g = P.svm_predict(model)
        assert (g.__name__, g.signature, g.types, g.nin, g.nout) == ("svm_out", "(n)->()", ["f->f", "d->d"], 1, 1)
        assert fake.live() == 0  # nothing on the device before the first call
        res = g(rows)
        assert res.shape == (N_WF,) and res.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_svm_rows" and len(call) == 21
        assert call[1][3] == N_WF * LEN * rows.itemsize and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == code
        assert [c[3] for c in call[7:12]] == [N_SV * LEN * 8, N_SV * 8, N_SV * PAIRS * 8, PAIRS * 8, K * 8]
        assert call[12:16] == [N_SV, K, 1, model["gamma"]] and call[16][3] == N_WF * np.dtype(loop).itemsize and call[17] is None and call[18] == 0
        assert call[19] is None and call[20] == "byref"
        assert fake.live() == 5  # the model stays with the processor
        # ... as bound: the arrays of svm_cases.host_arrays, bit for bit
        for d, want in zip(g.device_arrays, sc.host_arrays(model)):
            assert np.array_equal(d.to_numpy().reshape(want.shape), want)
        held = [c[1] for c in call[7:12]]
        one = g(rows[0])
        assert np.ndim(one) == 0 and [c[1] for c in fake.calls[-1][7:12]] == held and fake.calls[-1][3] == 1 and fake.live() == 5  # no new upload
        o = np.zeros(N_WF, dtype=loop)
        assert g(rows, o) is o
        for d in g.device_arrays:
            d.free()


def test_the_null_processor_and_calls_that_never_reach_the_library(tmp_path):
    from dspeed_amd import processors as P

    with _installed() as fake:
        null = P.svm_predict(0)
        out = null(np.ones((N_WF, LEN), np.float32))
        assert out.shape == (N_WF,) and out.dtype == np.float32 and np.isnan(out).all() and np.isnan(null(np.ones(LEN))) and null.model is None
        o = np.zeros(N_WF, np.float32)
        assert null(np.ones((N_WF, LEN), np.float32), o) is o and np.isnan(o).all()
        g = P.svm_predict(_model())
        with pytest.raises(ValueError, match="^svm_predict: the rows hold 15 samples, the model's support vectors 16$"):
            g(np.ones((N_WF, LEN - 1), np.float32))
        with pytest.raises(NotImplementedError, match="^svm_predict: float32 rows \\(the float32 loop\\) or float64 rows \\(the float64 loop\\), not int16$"):
            g(np.ones((N_WF, LEN), np.int16))
        with pytest.raises(TypeError, match="takes w_in and label_out"):
            g()
        assert fake.calls == [] and fake.live() == 0
    for kernel in ("poly", "sigmoid", "precomputed"):
        with pytest.raises(NotImplementedError, match=f"svm_predict: the kernel function '{kernel}' is not implemented on the device: 'rbf' and 'linear' are"):
            P.svm_predict(dict(_model(), kernel=kernel))
    with pytest.raises(TypeError, match="svm_predict: the class labels are .*; the label of a row is a number"):
        P.svm_predict(dict(_model(), classes=np.array(["a", "b", "c", "d"])))
    with pytest.raises(TypeError, match="svm_predict: 'list' is no fitted sklearn.svm.SVC"):
        P.svm_predict([1, 2])
    with pytest.raises(ValueError, match="svm_predict: the model's arrays do not fit each other"):
        P.svm_predict(dict(_model(), intercept=np.zeros(5)))
    with pytest.raises(NotImplementedError, match=f"^svm_predict: {sc.LIMITS} \\(n = 16, 24 classes given\\)$"):
        P.svm_predict(sc.synthetic(1, 16, 30, 24, "rbf"))


def test_the_npz_route_needs_no_scikit_learn(tmp_path, monkeypatch):
    from dspeed_amd import processors as P

    model = _model()
    path = str(tmp_path / "model.npz")
    np.savez(path, **model)
    monkeypatch.setitem(__import__("sys").modules, "sklearn", None)  # (an import of it would raise)
    g = P.svm_predict(path)
    for field in ("support_vectors", "n_support", "dual_coef", "intercept", "classes"):
        assert np.array_equal(g.model[field], model[field])
    assert g.model["kernel"] == "rbf" and g.model["gamma"] == model["gamma"]
    pickled = str(tmp_path / "model.pkl")
    with open(pickled, "wb") as f:
        pickle.dump({"not": "opened"}, f)
    with pytest.raises(ImportError, match="is a pickle of a scikit-learn SVC, and scikit-learn is not installed where the chain is built"):
        P.svm_predict(pickled)


def test_the_pickle_route_and_the_refusals_of_a_fitted_model(tmp_path):
    pytest.importorskip("sklearn")
    from sklearn.svm import SVC, LinearSVC

    from dspeed_amd import processors as P

    rng = np.random.default_rng(3)
    y = rng.integers(0, 3, 90)
    x = rng.standard_normal((90, 6)) + 2.0 * y[:, None]
    svc = SVC(kernel="rbf", gamma="scale").fit(x, np.array([1, 3, 5])[y])
    path = str(tmp_path / "svm.pkl")
    with open(path, "wb") as f:
        pickle.dump(svc, f)
    g = P.svm_predict(path)
    arrays = P.svm_model_arrays(svc)
    assert sorted(arrays) == sorted(("kernel", "gamma", "support_vectors", "n_support", "dual_coef", "intercept", "classes"))
    assert np.array_equal(g.model["dual_coef"], svc._dual_coef_) and np.array_equal(g.model["intercept"], svc._intercept_) and g.model["gamma"] == svc._gamma
    rows = rng.standard_normal((30, 6)).astype(np.float32) + 2.0
    assert np.array_equal(sc.emulate(g.model, rows)[0], svc.predict(rows.astype(np.float64)).astype(np.float64))
    P.save_svm_model(str(tmp_path / "svm.npz"), svc)
    again = P.svm_predict(str(tmp_path / "svm.npz"))
    assert all(np.array_equal(again.model[f], g.model[f]) for f in ("support_vectors", "n_support", "dual_coef", "intercept", "classes"))
    assert np.array_equal(P.svm_predict(svc).model["support_vectors"], svc.support_vectors_)
    two = SVC(kernel="linear").fit(x, y > 0)  # (bool classes are numbers; the underscored attributes carry libsvm's sign)
    assert np.array_equal(P.svm_model_arrays(two)["dual_coef"], -two.dual_coef_) and np.array_equal(P.svm_model_arrays(two)["intercept"], -two.intercept_)
    for kernel in ("poly", "sigmoid"):
        with pytest.raises(NotImplementedError, match=f"svm_predict: the kernel function '{kernel}' is not implemented on the device"):
            P.svm_model_arrays(SVC(kernel=kernel).fit(x, y))
    with pytest.raises(NotImplementedError, match="svm_predict: the kernel function 'given as a callable' is not implemented on the device"):
        P.svm_model_arrays(SVC(kernel=lambda a, b: a @ b.T).fit(x, y))
    with pytest.raises(NotImplementedError, match="svm_predict: break_ties=True is not implemented on the device"):
        P.svm_model_arrays(SVC(break_ties=True, decision_function_shape="ovr").fit(x, y))
    with pytest.raises(TypeError, match="svm_predict: the class labels are .*; the label of a row is a number"):
        P.svm_model_arrays(SVC().fit(x, np.array(["a", "b", "c"])[y]))
    with pytest.raises(TypeError, match="svm_predict: 'SVC' is no fitted sklearn.svm.SVC"):
        P.svm_model_arrays(SVC())
    with pytest.raises(TypeError, match="svm_predict: 'LinearSVC' is no fitted sklearn.svm.SVC"):
        P.svm_model_arrays(LinearSVC().fit(x, y))


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _recipe(tmp_path, init=("db.svm_file",), module=M):
    model = sc.synthetic(77, 64, 40, 3, "rbf", classes=(1, 3, 5))
    path = str(tmp_path / "model.npz")
    np.savez(path, **model)
    rng = np.random.default_rng(1)
    db = {"means": rng.standard_normal(64).tolist(), "variances": rng.uniform(1, 2, 64).tolist(), "svm_file": f"'{path}'"}
    procs = {"dwt": {"function": "discrete_wavelet_transform", "module": M, "args": ["waveform", 2, "'h'", "'a'", "dwt(64)"]},
             "dwt_norm": {"function": "normalisation_layer", "module": M, "args": ["dwt", "db.means", "db.variances", "dwt_norm"]},
             "label": {"function": "svm_predict", "module": module, "args": ["dwt_norm", "label"], "init_args": list(init)},
             "is_clean": "where(label == 3, 1, 0)"}
    return procs, db, model, path


def test_the_stage_list_of_a_cleaning_recipe(tmp_path):
    from dspeed_amd.processing_chain import build_processing_chain

    tb = {"waveform": np.zeros((9, 256), np.float32)}
    L, S, SS = _lib.OP_LOAD, _lib.OP_STORE, _lib.OP_STORE_SCALAR
    for module in (M, f"{M}.svm"):
        procs, db, model, path = _recipe(tmp_path, module=module)
        chain, _, out = build_processing_chain({"outputs": ["label", "is_clean"], "processors": procs}, tb, db_dict=db)
        stages = _stages(chain)
        whats = [s[0] for s in stages]
        assert whats.index("dwt -> HBM") < whats.index("normalisation_layer dwt_norm on rows") < whats.index("svm_predict label on rows")  # by dependency
        assert stages[whats.index("svm_predict label on rows")][1:] == (KERNEL, [L, _lib.OP_SVM_PREDICT, SS])
        st = chain._stages[whats.index("svm_predict label on rows")]
        assert [(io[1], io[3]) for io in st["program"].io] == [(_lib.IO_WF_IN, 64), (_lib.IO_TAPS, 40 * 64), (_lib.IO_TAPS, 40), (_lib.IO_TAPS, 40 * 3), (_lib.IO_TAPS, 3),
                                                                  (_lib.IO_TAPS, 3), (_lib.IO_SCALAR_OUT, 1)]
        consts = st["consts"]
        assert all(v.dtype == np.float64 and v.ndim == 1 for v in consts.values())
        for got, want in zip((consts[f"taps:{name}#label"] for name in ("support_vectors", "sv_norms", "coefficients", "intercepts", "classes")), sc.host_arrays(model)):
            assert np.array_equal(got, want.reshape(-1))
        assert out["label"].shape == (9,) and out["label"].dtype == np.float32 and out["is_clean"].shape == (9,)  # the label feeds a later expression
    # the file as a character constant; the null processor: nothing launched, NaN for every row
    procs, db, model, path = _recipe(tmp_path, init=(f"'{path}'",))
    chain, _, out = build_processing_chain({"outputs": ["label"], "processors": procs}, tb, db_dict=db)
    assert "svm_predict label on rows" in [s[0] for s in _stages(chain)]
    procs, db, model, path = _recipe(tmp_path, init=(0,))
    del procs["is_clean"]
    chain, _, out = build_processing_chain({"outputs": ["label"], "processors": procs}, tb, db_dict=db)
    assert not chain._stages and out["label"].dtype == np.float32 and np.isnan(out["label"]).all() and out["label"].shape == (9,)
    null = {"label": {"function": "svm_predict", "module": M, "args": ["waveform", "label"], "init_args": [0]}}
    chain, _, out = build_processing_chain({"outputs": ["label"], "processors": null}, {"waveform": np.zeros((9, 256), np.float64)}, db_dict=db)
    assert out["label"].dtype == np.float64 and np.isnan(out["label"]).all()  # (the loop's type, as the staged label has it)


def test_recipe_refusals_by_name(tmp_path):
    from dspeed_amd.processing_chain import build_processing_chain

    tb = {"waveform": np.zeros((9, 256), np.float32)}

    def build(procs, db, outputs=("label",), table=None):
        return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or tb, db_dict=db)

    procs, db, model, path = _recipe(tmp_path)
    del procs["label"]["init_args"]
    with pytest.raises(ProcessingChainError, match="^svm_predict \\(label\\): init_args holds the file of the fitted SVC \\(or 0\\), as the factory takes it$"):
        build(procs, db)
    procs, db, model, path = _recipe(tmp_path)
    procs["label"]["args"][0] = "dwt"
    procs["dwt"]["args"][1] = 1  # rows of 128 samples against a model of 64
    procs["dwt"]["args"][4] = "dwt(128)"
    with pytest.raises(ProcessingChainError, match="^svm_predict \\(label\\): 'dwt' holds 128 samples, the model's support vectors 64$"):
        build(procs, db)
    np.savez(path, **sc.synthetic(1, 64, 30, 24, "rbf"))
    procs["label"]["args"][0], procs["dwt"]["args"][1], procs["dwt"]["args"][4] = "dwt", 2, "dwt(64)"
    with pytest.raises(NotImplementedError, match=f"^svm_predict \\(label\\): {sc.LIMITS} \\(n = 64, 24 classes given\\)$"):
        build(procs, db)
    # init_args on a processor that is no factory: the refusal as it was, word for word
    with pytest.raises(NotImplementedError, match="^log_check \\(wf_log\\): init_args builds a processor from a factory; on the device path only poly_fit is one$"):
        build({"wf_log": {"function": "log_check", "module": M, "args": ["waveform", "wf_log"], "init_args": [1]}}, db, outputs=("wf_log",))
