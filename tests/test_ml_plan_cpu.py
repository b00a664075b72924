"""The planner's, the registry's and the recipe compiler's part of the neural-network layers without a device (dsp_chain_plan):
DSP_OP_NORMALISE and DSP_OP_DENSE have one route -- dsp_dense_kernel, whatever the switches say --, three program shapes and every
refusal by name; the opcodes are appended; the five processors are attributes of the registry listed in ``ML``; what a call hands to the
library (against a subclass of tests/fake_dsp_lib.FakeLib); the stage list of the reference's docstring recipe."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

import fake_dsp_lib
import ml_cases as mc
from dspeed_amd import _lib
from dspeed_amd.chain import Scalar, plan
from dspeed_amd.errors import ProcessingChainError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = "dspeed.processors"
KERNEL = mc.KERNEL
F64 = dict(rows=np.float64, loop=np.float64)
NAMES = ("normalisation_layer", "dense_layer_no_bias", "dense_layer_with_bias", "classification_layer_no_bias", "classification_layer_with_bias")
SHAPE = ("DSP_OP_NORMALISE / DSP_OP_DENSE \\(normalisation_layer, dense_layer_\\*, classification_layer_\\*\\) run on dsp_dense_kernel only, on rows in "
         "memory: the program must be exactly LOAD, \\[NORMALISE,\\] DENSE, STORE; LOAD, \\[NORMALISE,\\] DENSE, STORE_SCALAR; or LOAD, NORMALISE, STORE")


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_shapes_take_the_dense_kernel_whatever_the_switches_say(monkeypatch):
    def all_of_them():
        for rows in ("f32", "f64"):
            kw = F64 if rows == "f64" else {}
            dt = mc.LOOPS[rows]
            for k, (n, m, _count) in enumerate(mc.shapes(rows)):
                act, bias = mc.variant(k)
                assert plan(mc.program(n, m, act, bias, norm=k % 3 == 0, **kw), dt)["kernel"] == KERNEL
            assert plan(mc.program(100, 1, "s", classify=True, **kw), dt)["kernel"] == KERNEL
            assert plan(mc.program(100, 1, "t", bias=False, norm=True, classify=True, **kw), dt)["kernel"] == KERNEL
            assert plan(mc.program(100, 1, norm=True, dense=False, **kw), dt)["kernel"] == KERNEL
        assert plan(mc.program(1000, 33, rows=np.int16))["kernel"] == KERNEL
        assert plan(mc.program(1000, 33, rows=np.uint16, offset=3, row_stride=1007, out_stride=40))["kernel"] == KERNEL
        assert plan(mc.program(7, 256, act_code=0))["kernel"] == KERNEL and plan(mc.program(7, 2, act_code=300))["kernel"] == KERNEL  # (any character: NaN outputs)

    all_of_them()
    for switch in ("DSPEED_HIP_NO_FUSED", "DSPEED_HIP_NO_ROW_REDUCTIONS", "DSPEED_HIP_NO_TEAMS"):
        monkeypatch.setenv(switch, "1")
    all_of_them()


def test_the_geometry_the_case_book_assumes_is_the_headers():
    header = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_kernels.h")).read()
    assert "constexpr int WAVES = 4, WAVE_ROWS = 16, TILE_ROWS = WAVES * WAVE_ROWS, BLOCK = 16, DEPTH = 4;" in header
    assert "constexpr int chunk(int esz) { return 256 / esz; }" in header and "constexpr int N_MAX = 16384, M_MAX = 256" in header
    assert (mc.chunk(np.float32), mc.chunk(np.float64)) == (64, 32)
    assert mc.lds_bytes(256, 4) == mc.lds_bytes(256, 8) == 87040 and mc.lds_bytes(1, 4) == (64 * 16 + 64 * 68) * 4


def test_the_limits_by_name_in_one_text():
    assert (_lib.DENSE_N_MAX, _lib.DENSE_M_MAX) == (mc.N_MAX, mc.M_MAX) == (16384, 256)
    header = open(os.path.join(ROOT, "dspeed_amd", "csrc", "dsp_program.h")).read()
    for line in ("#define DSP_DENSE_N_MAX 16384", "#define DSP_DENSE_M_MAX 256", '#define DSP_DENSE_LIMITS_TEXT "layers of up to %d inputs and %d outputs"'):
        assert line in header
    from dspeed_amd import processors

    assert processors.DENSE_LIMITS == mc.LIMITS
    plan(mc.program(16384, 256)), plan(mc.program(16384, 256, **F64), np.float64), plan(mc.program(16384, 1, classify=True))
    plan(mc.program(16384, 1, norm=True, dense=False))
    for n, m in ((16385, 4), (1 << 19, 1), (10, 257), (16384, 1000)):
        with pytest.raises(NotImplementedError, match=f"dense_layer: {mc.LIMITS} \\(n = {n}, m = {m} given\\)"):
            plan(mc.program(n, m))
        with pytest.raises(NotImplementedError, match=f"dense_layer: {mc.LIMITS} \\(n = {n}, m = {m} given\\)"):
            plan(mc.program(n, m, **F64), np.float64)
    with pytest.raises(NotImplementedError, match=f"dense_layer: {mc.LIMITS} \\(n = 16385, m = 1 given\\)"):
        plan(mc.program(16385, 1, classify=True))
    with pytest.raises(NotImplementedError, match=f"normalisation_layer: {mc.LIMITS} \\(n = 16385 given\\)"):
        plan(mc.program(16385, 1, norm=True, dense=False))


def test_any_other_program_with_the_ops_is_refused_by_name():
    p = mc.program(100, 17)
    p.ops.pop()  # no store
    with pytest.raises(NotImplementedError, match=SHAPE):
        plan(p)
    p = mc.program(100, 17)
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match=SHAPE):
        plan(p)
    p = mc.program(100, 17)
    p.n_sregs = 4
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=1)  # a second reader of the outputs
    with pytest.raises(NotImplementedError, match=SHAPE):
        plan(p)
    p = mc.program(100, 100, norm=True)
    p.ops[1], p.ops[2] = p.ops[2], p.ops[1]  # the normalisation behind the layer
    with pytest.raises(NotImplementedError, match=SHAPE):
        plan(p)
    p = mc.program(100, 20)
    w2 = p.add_io("kernel2", _lib.IO_TAPS, np.float32, 20 * 3, 0, 0)
    o2 = p.add_slot(3)
    p.ops.insert(2, (_lib.OP_DENSE, o2, 1, w2, (ord("s"), -1, 20, 3), ()))  # two layers in one program: out of scope
    with pytest.raises(NotImplementedError, match=SHAPE):
        plan(p)
    p = mc.program(100, 1, classify=True)
    p.ops[-1] = (_lib.OP_STORE_SCALAR, 0, 0, p.ops[-1][3], (0,), ())
    p.n_sregs = 2
    p.ops[1] = p.ops[1][:1] + (1,) + p.ops[1][2:]  # the value goes to register 1, register 0 is stored
    with pytest.raises(NotImplementedError, match="DSP_OP_NORMALISE / DSP_OP_DENSE.*the result is stored once, whole, in the loop's type"):
        plan(p)
    for rows in (np.int32, np.uint32):
        with pytest.raises(NotImplementedError, match="DSP_OP_NORMALISE / DSP_OP_DENSE.*the float32 loop takes float32, int16 or uint16 rows, the float64 loop float64 rows"):
            plan(mc.program(100, 17, rows=rows, loop=np.float64), np.float64)
    with pytest.raises(ValueError, match="float64 rows select the float64 loop"):  # (every program's rule)
        plan(mc.program(100, 17, rows=np.float64))


def test_malformed_operands_are_refused_by_name():
    p = mc.program(100, 17)
    p.ops[1] = p.ops[1][:1] + (0,) + p.ops[1][2:]  # destination = source
    with pytest.raises(ValueError, match="bad DENSE \\(src: the slot of the row; dst: another slot, of ip\\[3\\] = m samples, or with ip\\[3\\] = 0 a scalar register\\)"):
        plan(p)
    p = mc.program(100, 17)
    p.ops[1] = p.ops[1][:4] + ((ord("r"), -1, 99, 17),) + p.ops[1][5:]
    with pytest.raises(ValueError, match="DENSE: ip\\[2\\] is the length of the row \\(100\\), ip\\[3\\] that of the output slot or 0 \\(99 and 17 given\\)"):
        plan(p)
    p = mc.program(100, 17)
    p.ops[1] = p.ops[1][:4] + ((ord("r"), -1, 100, 16),) + p.ops[1][5:]
    with pytest.raises(ValueError, match="DENSE: ip\\[2\\] is the length of the row"):
        plan(p)
    p = mc.program(100, 17)
    p.io[1] = p.io[1][:3] + (100 * 16,) + p.io[1][4:]  # weights of another shape
    with pytest.raises(ValueError, match="dense_layer: the weights \\(io\\) are a DSP_IO_TAPS binding of n \\* m = 100 \\* 17 values, row-major"):
        plan(p)
    p = mc.program(100, 17)
    p.io[2] = p.io[2][:3] + (16,) + p.io[2][4:]
    with pytest.raises(ValueError, match="dense_layer: the bias \\(ip\\[1\\]\\) is a DSP_IO_TAPS binding of m = 17 values, or -1"):
        plan(p)
    p = mc.program(100, 17)
    p.ops[1] = p.ops[1][:4] + ((ord("r"), 0, 100, 17),) + p.ops[1][5:]  # the rows as the bias
    with pytest.raises(ValueError, match="dense_layer: the bias"):
        plan(p)
    p = mc.program(100, 17, norm=True)
    p.io[2] = p.io[2][:3] + (99,) + p.io[2][4:]
    with pytest.raises(ValueError, match="normalisation_layer: means \\(io\\) and variances \\(ip\\[0\\]\\) are DSP_IO_TAPS bindings of len\\(x_in\\) = 100 values"):
        plan(p)
    p = mc.program(100, 17, norm=True)
    p.ops[1] = p.ops[1][:4] + ((77,),) + p.ops[1][5:]
    with pytest.raises(ValueError, match="normalisation_layer: means"):
        plan(p)
    p = mc.program(100, 17, norm=True)
    p.add_slot(100)
    p.ops[1] = p.ops[1][:1] + (2,) + p.ops[1][2:]  # not in place
    with pytest.raises(ValueError, match="bad NORMALISE \\(src = dst: the slot of the row, normalised in place\\)"):
        plan(p)
    p = mc.program(100, 1, classify=True)
    p.ops[1] = p.ops[1][:1] + (5,) + p.ops[1][2:]
    with pytest.raises(ValueError, match="bad DENSE"):
        plan(p)


def test_the_opcodes_are_appended_and_the_registry_lists_the_processors_apart():
    from dspeed_amd import processors
    from dspeed_amd.language import _PROCESSOR_FILES, _SIGS, module_accepted

    assert (_lib.OP_INTERP_UPSAMPLE, _lib.OP_NORMALISE, _lib.OP_DENSE) == (42, 43, 44)
    header = open(os.path.join(ROOT, "include", "dspeed_hip.h")).read()
    assert "#define DSP_OP_NORMALISE 43" in header and "#define DSP_OP_DENSE 44" in header and "#define DSP_OP_INTERP_UPSAMPLE 42" in header
    assert not re.search(r"dsp_(dense|normalisation)_rows_f(32|64)", header)  # one entry each, the loop an argument
    assert processors.ML == NAMES
    others = set(processors.__all__) | set(processors.SPECTRAL) | set(processors.ORDER) | set(processors.RESAMPLING) | set(_PROCESSOR_FILES)
    assert not set(processors.ML) & others
    want = {"normalisation_layer": ("(n),(n),(n)->(n)", ["fff->f", "ddd->d"], 3, 1),
            "dense_layer_no_bias": ("(n),(n,m),()->(m)", ["ffb->f", "ddb->d"], 3, 1),
            "dense_layer_with_bias": ("(n),(n,m),(m),()->(m)", ["fffb->f", "dddb->d"], 4, 1),
            "classification_layer_no_bias": ("(n),(n),()->()", ["ffb->f", "ddb->d"], 3, 1),
            "classification_layer_with_bias": ("(n),(n),(),()->()", ["fffb->f", "dddb->d"], 4, 1)}
    for name, (sig, types, nin, nout) in want.items():
        g = getattr(processors, name)
        assert (g.signature, g.types, g.nin, g.nout, g.__name__) == (sig, types, nin, nout, name)
        assert name in _SIGS and len(_SIGS[name]) == nin + nout
        assert module_accepted(M, name) and module_accepted(f"{M}.ml", name) and module_accepted("dspeed_amd.processors", name)
        assert not module_accepted(f"{M}.sort", name)
    assert not module_accepted(f"{M}.ml", "sort")
    L = ctypes.CDLL(_lib.LIB_PATH)
    for entry in ("dsp_dense_rows", "dsp_normalisation_rows"):
        assert hasattr(L, entry) and entry in _lib.EXPORTS and re.search(rf"\bint {entry}\(", header)
    # the header's argument lists are the ctypes table's
    for entry in ("dsp_dense_rows", "dsp_normalisation_rows"):
        decl = re.search(rf"\bint {entry}\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIG[entry])


# ---------------------------------------------------------------------------------------------------------------- what a call hands to the library
class _Fake(fake_dsp_lib.FakeLib):
    """the stand-in with the entries that name their loop in an argument instead of a suffix"""

    def dsp_dense_rows(self, *args):
        self.calls.append(["dsp_dense_rows"] + [self._name(a) for a in args])
        return 0

    def dsp_normalisation_rows(self, *args):
        self.calls.append(["dsp_normalisation_rows"] + [self._name(a) for a in args])
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


N_WF, LEN, OUT = 3, 16, 5


def _rows(dtype, shape=(N_WF, LEN)):
    return (np.arange(int(np.prod(shape))) % 7).astype(dtype).reshape(shape)


@pytest.mark.parametrize("dtype, code, loop_code, loop", [(np.float32, _lib.F32, _lib.F32, np.float32), (np.int16, _lib.I16, _lib.F32, np.float32),
                                                          (np.uint16, _lib.U16, _lib.F32, np.float32), (np.float64, _lib.F64, _lib.F64, np.float64)])
def test_the_arguments_of_a_call(dtype, code, loop_code, loop):
    """rows (pointer, type, count, length, stride), the loop's type, weights, bias or NULL, the activation, the output, its length (0: one
    value a row) and stride, the stream, the row of an error"""
    from dspeed_amd import processors as P
    from dspeed_amd.device import DeviceArray

    esz, isz = np.dtype(loop).itemsize, np.dtype(dtype).itemsize
    w, b = np.ones((LEN, OUT)), np.ones(OUT)  # (float64 on the host: cast to the loop's type on their way)
    with _installed() as fake:
        res = P.dense_layer_with_bias(_rows(dtype), w, b, "s")
        assert res.shape == (N_WF, OUT) and res.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_dense_rows" and len(call) == 15
        assert call[1] == ["ptr", 0, 0, N_WF * LEN * isz] and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7] == ["ptr", 1, 0, LEN * OUT * esz] and call[8] == ["ptr", 2, 0, OUT * esz] and call[9] == ord("s")
        assert call[10] == ["ptr", 3, 0, N_WF * OUT * esz] and call[11:13] == [OUT, OUT] and call[13] is None and call[14] == "byref"
        assert fake.live() == 0
        del fake.calls[:]
        o = np.zeros((N_WF, OUT), dtype=loop)
        assert P.dense_layer_no_bias(_rows(dtype), w, np.int8(ord("r")), o) is o  # written in place; the activation as the reference passes it
        (call,) = fake.calls
        assert call[8] is None and call[9] == ord("r") and call[11:13] == [OUT, OUT]
        # the classification layers: out_len 0, a value per row
        del fake.calls[:]
        res = P.classification_layer_with_bias(_rows(dtype), np.ones(LEN), 0.5, "t")
        assert res.shape == (N_WF,) and res.dtype == loop
        (call,) = fake.calls
        assert call[7][3] == LEN * esz and call[8][3] == esz and call[9] == ord("t") and call[10][3] == N_WF * esz and call[11] == 0
        del fake.calls[:]
        one = P.classification_layer_no_bias(_rows(dtype, (LEN,)), np.ones(LEN), "q")  # a 1-D call, a character the reference does not know
        assert np.ndim(one) == 0
        (call,) = fake.calls
        assert call[2:6] == [code, 1, LEN, LEN] and call[8] is None and call[9] == ord("q") and call[11] == 0
        # normalisation_layer
        del fake.calls[:]
        res = P.normalisation_layer(_rows(dtype), np.zeros(LEN), np.ones(LEN))
        assert res.shape == (N_WF, LEN) and res.dtype == loop
        (call,) = fake.calls
        assert call[0] == "dsp_normalisation_rows" and len(call) == 13 and call[2:6] == [code, N_WF, LEN, LEN] and call[6] == loop_code
        assert call[7][3] == call[8][3] == LEN * esz and call[9][3] == N_WF * LEN * esz and call[10] == LEN and call[11] is None
        assert fake.live() == 0
        # rows, weights and output on the device: their own memory, nothing staged
        del fake.calls[:]
        d, dw, do = DeviceArray.from_numpy(_rows(dtype)), DeviceArray.from_numpy(w.astype(loop)), DeviceArray((N_WF, OUT), loop)
        before = len(fake.device)
        assert P.dense_layer_no_bias(d, dw, "l", do) is do
        (call,) = fake.calls
        assert len(fake.device) == before and [call[1][1], call[7][1], call[10][1]] == [before - 3, before - 2, before - 1]
        d.free(), dw.free(), do.free()
        assert fake.live() == 0


def test_calls_that_never_reach_the_library():
    from dspeed_amd import processors as P

    f32 = np.float32
    w = np.ones((LEN, OUT), f32)
    with _installed() as fake:
        with pytest.raises(NotImplementedError, match="^dense_layer_no_bias: the float64 loop takes float64 rows on the device$"):
            P.dense_layer_no_bias(_rows(np.int32), w, "r")
        with pytest.raises(NotImplementedError, match="^dense_layer_no_bias: activation_func is a constant of the call on the device, not a per-event value$"):
            P.dense_layer_no_bias(_rows(f32), w, np.array([ord("r"), ord("s"), ord("r")], np.int8))
        with pytest.raises(ValueError, match="^dense_layer_no_bias: kernel has shape \\(15, 5\\), expected \\(16, m\\)$"):
            P.dense_layer_no_bias(_rows(f32), w[:15], "r")
        with pytest.raises(ValueError, match="^dense_layer_with_bias: bias has shape \\(4,\\), expected \\(5,\\)$"):
            P.dense_layer_with_bias(_rows(f32), w, np.ones(4, f32), "r")
        with pytest.raises(ValueError, match="^classification_layer_no_bias: kernel has shape \\(16, 5\\), expected \\(16,\\)$"):
            P.classification_layer_no_bias(_rows(f32), w, "r")
        with pytest.raises(NotImplementedError, match="^classification_layer_with_bias: bias is a constant of the call on the device, not a per-event value$"):
            P.classification_layer_with_bias(_rows(f32), w[:, 0], np.ones(N_WF, f32), "r")
        with pytest.raises(ValueError, match="^normalisation_layer: variances has shape \\(15,\\), expected \\(16,\\)$"):
            P.normalisation_layer(_rows(f32), np.zeros(LEN), np.ones(15))
        with pytest.raises(NotImplementedError, match=f"^dense_layer_no_bias: {mc.LIMITS} \\(n = 16385, m = 2 given\\)$"):
            P.dense_layer_no_bias(np.zeros((1, 16385), f32), np.zeros((16385, 2), f32), "r")
        with pytest.raises(NotImplementedError, match=f"^dense_layer_with_bias: {mc.LIMITS} \\(n = 4, m = 257 given\\)$"):
            P.dense_layer_with_bias(np.zeros((2, 4), np.float64), np.zeros((4, 257)), np.zeros(257), "r")
        with pytest.raises(NotImplementedError, match=f"^normalisation_layer: {mc.LIMITS} \\(n = 16385, m = 1 given\\)$"):
            P.normalisation_layer(np.zeros((1, 16385), f32), np.zeros(16385), np.ones(16385))
        with pytest.raises(ValueError, match="Outputs are not the right shape"):
            P.dense_layer_no_bias(_rows(f32), w, "r", np.zeros((N_WF, OUT + 1), f32))
        with pytest.raises(TypeError, match="takes 3 inputs and 1 outputs"):
            P.dense_layer_no_bias(_rows(f32), w)
        assert fake.calls == [] and fake.live() == 0


# ---------------------------------------------------------------------------------------------------------------- recipes
def _stages(chain):
    return [(st["what"], plan(st["program"])["kernel"], [op[0] for op in st["program"].ops]) for st in chain._stages]


def _recipe(module=M):
    """the reference's docstring example (ml.py:5-32), the second dense layer with weights of its own"""
    return {"layer_1": {"function": "normalisation_layer", "module": module, "args": ["wf_blsub", "db.mean", "db.variance", "layer_1"]},
            "layer_2": {"function": "dense_layer_with_bias", "module": module, "args": ["layer_1", "db.kernel", "db.bias", "'r'", "layer_2"]},
            "classifier": {"function": "dense_layer_with_bias", "module": module, "args": ["layer_2", "db.kernel_2", "db.bias_2", "'s'", "classifier"]}}


def _db(n=100, m=20, k=3):
    rng = np.random.default_rng(5)
    return {"mean": rng.normal(size=n).tolist(), "variance": rng.uniform(1, 2, n).tolist(), "kernel": rng.normal(size=(n, m)).tolist(),
            "bias": rng.normal(size=m).tolist(), "kernel_2": rng.normal(size=(m, k)).tolist(), "bias_2": rng.normal(size=k).tolist(),
            "kernel_1d": rng.normal(size=m).tolist()}


def _table(n=100, rows=12, dtype=np.float32):
    from dspeed_amd.processing_chain import WaveformInput

    rng = np.random.default_rng(7)
    return {"wf_blsub": WaveformInput(rng.normal(size=(rows, n)).astype(dtype), 16.0), "bl": rng.uniform(-1, 1, rows).astype(np.float32)}


L, N, D, S, SS = _lib.OP_LOAD, _lib.OP_NORMALISE, _lib.OP_DENSE, _lib.OP_STORE, _lib.OP_STORE_SCALAR


def test_the_stage_list_of_the_docstring_recipe():
    from dspeed_amd.processing_chain import build_processing_chain

    for module in (M, f"{M}.ml"):
        chain, _, out = build_processing_chain({"outputs": ["classifier"], "processors": _recipe(module)}, _table(), db_dict=_db())
        # the normalisation is folded into the first layer's loads: one fused launch for the pair, one for the second layer
        assert _stages(chain) == [("normalisation_layer layer_1 + dense_layer_with_bias layer_2 in one launch on rows", KERNEL, [L, N, D, S]),
                                  ("dense_layer_with_bias classifier on rows", KERNEL, [L, D, S])]
        st = chain._stages[0]["program"]
        assert [(io[1], io[3]) for io in st.io] == [(_lib.IO_WF_IN, 100), (_lib.IO_TAPS, 100), (_lib.IO_TAPS, 100), (_lib.IO_TAPS, 2000), (_lib.IO_TAPS, 20), (_lib.IO_WF_OUT, 20)]
        assert st.ops[2][4] == (ord("r"), 4, 100, 20) and st.ops[1][3] == 1 and st.ops[1][4][0] == 2
        consts = chain._stages[0]["consts"]
        assert all(v.dtype == np.float32 and v.ndim == 1 for v in consts.values()) and sorted(len(v) for v in consts.values()) == [20, 100, 100, 2000]
        assert out["classifier"].shape == (12, 3) and out["classifier"].dtype == np.float32
        st2 = chain._stages[1]["program"]
        assert st2.ops[1][4] == (ord("s"), 2, 20, 3) and st2.io[0][0] == "in:layer_2"
    # the normalisation launched on its own when it is an output
    chain, _, out = build_processing_chain({"outputs": ["classifier", "layer_1"], "processors": _recipe()}, _table(), db_dict=_db())
    assert _stages(chain) == [("normalisation_layer layer_1 on rows", KERNEL, [L, N, S]), ("dense_layer_with_bias layer_2 on rows", KERNEL, [L, D, S]),
                              ("dense_layer_with_bias classifier on rows", KERNEL, [L, D, S])]
    assert out["layer_1"].shape == (12, 100)
    # ... or when something that is no layer reads it
    procs = _recipe()
    procs["tp_min, tp_max, wf_min, wf_max"] = {"function": "min_max", "module": M, "args": ["layer_1", "tp_min", "tp_max", "wf_min", "wf_max"]}
    chain, _, out = build_processing_chain({"outputs": ["classifier", "wf_max"], "processors": procs}, _table(), db_dict=_db())
    assert [s[2] for s in _stages(chain)][:3] == [[L, N, S], [L, D, S], [L, D, S]]


def test_classification_layers_sources_and_constant_forms():
    from dspeed_amd.processing_chain import build_processing_chain

    procs = _recipe()
    procs["score"] = {"function": "classification_layer_with_bias", "module": M, "args": ["layer_2", "db.kernel_1d", 0.25, "'t'", "score"]}
    procs["score_2"] = {"function": "classification_layer_no_bias", "module": f"{M}.ml", "args": ["layer_1", "[" + ", ".join(["0.5"] * 100) + "]", "'q'", "score_2"]}
    chain, _, out = build_processing_chain({"outputs": ["score", "score_2"], "processors": procs}, _table(), db_dict=_db())
    stages = _stages(chain)
    assert ("normalisation_layer layer_1 + classification_layer_no_bias score_2 in one launch on rows", KERNEL, [L, N, D, SS]) in stages
    assert ("dense_layer_with_bias score on rows".replace("dense_layer", "classification_layer"), KERNEL, [L, D, SS]) in stages
    assert [s[2] for s in stages].count([L, N, D, S]) == 1 and out["score"].shape == (12,) and out["score"].dtype == np.float32
    # a waveform the program computes is written to memory first; a recipe entry holding the constant array
    first = {"wf_sub": {"function": "bl_subtract", "module": M, "args": ["wf_blsub", "bl", "wf_sub"]}, "weights": str(_db()["kernel"])}
    first["layer"] = {"function": "dense_layer_no_bias", "module": M, "args": ["wf_sub", "weights", "'m'", "layer"]}
    chain, _, out = build_processing_chain({"outputs": ["layer"], "processors": first}, _table(), db_dict=_db())
    whats = [s[0] for s in _stages(chain)]
    assert whats.index("wf_sub -> HBM") < whats.index("dense_layer_no_bias layer on rows") and out["layer"].shape == (12, 20)
    # a declared output of the kernel's width
    one = {"layer": {"function": "dense_layer_no_bias", "module": M, "args": ["wf_blsub", "db.kernel", "'m'", "layer(20)"]}}
    assert build_processing_chain({"outputs": ["layer"], "processors": one}, _table(), db_dict=_db())[2]["layer"].shape == (12, 20)


def test_recipe_refusals_by_name(monkeypatch):
    from dspeed_amd.processing_chain import build_processing_chain

    def build(procs, table=None, outputs=("layer",), db=None):
        return build_processing_chain({"outputs": list(outputs), "processors": procs}, table or _table(), db_dict=db or _db())

    def one(args, fn="dense_layer_no_bias", module=M):
        return {"layer": {"function": fn, "module": module, "args": args}}

    build(one(["wf_blsub", "db.kernel", "'r'", "layer"]))
    with pytest.raises(ProcessingChainError, match="dense_layer_no_bias \\(layer\\): 'layer' holds 21 samples, the kernel has 20 columns"):
        build(one(["wf_blsub", "db.kernel", "'r'", "layer(21)"]))
    with pytest.raises(ProcessingChainError, match="dense_layer_no_bias \\(layer\\): 'wf_blsub' holds 100 samples, kernel has shape \\(20, 3\\)"):
        build(one(["wf_blsub", "db.kernel_2", "'r'", "layer"]))
    with pytest.raises(ProcessingChainError, match="dense_layer_no_bias \\(layer\\): kernel is a 2-dimensional array of numbers, not float64 of shape \\(100,\\)"):
        build(one(["wf_blsub", "db.mean", "'r'", "layer"]))
    with pytest.raises(ProcessingChainError, match="dense_layer_with_bias \\(layer\\): 'wf_blsub' holds 100 samples, bias holds 3 values"):
        build(one(["wf_blsub", "db.kernel", "db.bias_2", "'r'", "layer"], "dense_layer_with_bias"))
    with pytest.raises(NotImplementedError, match="dense_layer_no_bias \\(layer\\): kernel is a constant array .* not a per-event value"):
        build(one(["wf_blsub", "bl", "'r'", "layer"]))
    with pytest.raises(NotImplementedError, match="classification_layer_with_bias \\(layer\\): bias is a constant array .* not a per-event value"):
        build(one(["wf_blsub", "db.mean", "bl", "'r'", "layer"], "classification_layer_with_bias"))
    tb = _table()
    tb["which"] = np.full(12, ord("r"), np.int8)
    with pytest.raises(NotImplementedError, match="dense_layer_no_bias \\(layer\\): the activation function is a constant of the kernel, not a per-event value"):
        build(one(["wf_blsub", "db.kernel", "which", "layer"]), tb)
    big = {"kernel": np.zeros((16385, 2)).tolist(), "wide": np.zeros((100, 257)).tolist(), "mean": np.zeros(16385).tolist(), "variance": np.ones(16385).tolist()}
    with pytest.raises(NotImplementedError, match=f"dense_layer_no_bias \\(layer\\): {mc.LIMITS} \\(n = 16385, m = 2 given\\)"):
        build(one(["wf_blsub", "db.kernel", "'r'", "layer"]), _table(16385, 2), db=big)
    with pytest.raises(NotImplementedError, match=f"dense_layer_no_bias \\(layer\\): {mc.LIMITS} \\(n = 100, m = 257 given\\)"):
        build(one(["wf_blsub", "db.wide", "'r'", "layer"]), db=big)
    with pytest.raises(NotImplementedError, match=f"normalisation_layer \\(layer\\): {mc.LIMITS} \\(n = 16385, m = 1 given\\)"):
        build(one(["wf_blsub", "db.mean", "db.variance", "layer"], "normalisation_layer"), _table(16385, 2), db=big)
    with pytest.raises(Exception, match="dense_layer_no_bias"):
        build(one(["wf_blsub", "db.kernel", "'r'", "layer"], module=f"{M}.sort"))  # not the processor's file
    with pytest.raises(NotImplementedError, match="dense_layer_no_bias in a recipe whose loop type is float64"):
        build(one(["wf_blsub", "db.kernel", "'r'", "layer"]), _table(dtype=np.float64))
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="dense_layer_no_bias runs as a stage ahead of the program.*DSPEED_HIP_NO_STAGES"):
        build(one(["wf_blsub", "db.kernel", "'r'", "layer"]))
