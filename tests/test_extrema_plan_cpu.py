"""The planner's part of get_multi_local_extrema without a device (dsp_chain_plan): DSP_OP_MULTI_EXTREMA has one route -- its own kernel,
whatever the switches say --, every other program that holds the op is refused by name, the constant-only DSPFatal conditions of the
reference carry its texts, and the registry and the C ABI know the processor."""
import ctypes

import numpy as np
import pytest

from dspeed_amd import _lib
from dspeed_amd.chain import Program, Scalar, plan
from dspeed_amd.errors import DSPFatal


def program(n=513, m=20, direction=0, deltas=(5.0, 5.0), dtype=np.float32, count_dtype=np.uint32, column=False, stride=None):
    p = Program()
    p.slots = [n, m, m]
    p.n_sregs = 2
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dtype, n, 0, stride or n))
    loop = np.float32 if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.int16), np.dtype(np.uint16)) else np.float64
    d_max = Scalar.input(p.add_io("d_max", _lib.IO_SCALAR_IN, loop)) if column else Scalar.const(deltas[0])
    p.add_op(_lib.OP_MULTI_EXTREMA, dst=1, src=0, ip=(direction, 2, 0), sp=(d_max, Scalar.const(deltas[1]), Scalar.const(-np.inf), Scalar.const(np.inf)))
    p.add_op(_lib.OP_STORE, src=1, io=p.add_io("vt_max", _lib.IO_WF_OUT, loop, m))
    p.add_op(_lib.OP_STORE, src=2, io=p.add_io("vt_min", _lib.IO_WF_OUT, loop, m))
    p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("n_max", _lib.IO_SCALAR_OUT, count_dtype), ip=(0,))
    p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("n_min", _lib.IO_SCALAR_OUT, count_dtype), ip=(1,))
    return p, loop


@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.uint16, np.float64, np.int32, np.uint32])
@pytest.mark.parametrize("direction", [0, 1, 3])
def test_the_program_runs_on_its_own_kernel(dtype, direction, monkeypatch):
    for column in (False, True):
        for n, stride in ((513, None), (512, 512), (512, 515)):
            p, loop = program(n=n, direction=direction, dtype=dtype, column=column, stride=stride)
            assert plan(p, loop)["kernel"] == "dsp_extrema_kernel"
    monkeypatch.setenv("DSPEED_HIP_NO_FUSED", "1")  # no interpreter op behind it: the switch that turns the specialised kernels off leaves it on
    p, loop = program(direction=direction, dtype=dtype)
    assert plan(p, loop)["kernel"] == "dsp_extrema_kernel"


def test_rows_longer_than_a_wavefront_s_lds_are_taken():
    """the kernel keeps nothing in LDS: float64 rows of 8192 samples with lists of 8191, float32 rows of 100 000 samples"""
    for n, m, dtype in ((8192, 8191, np.float64), (100000, 20, np.float32)):
        p, loop = program(n=n, m=m, dtype=dtype)
        assert plan(p, loop)["kernel"] == "dsp_extrema_kernel"


def test_any_other_program_with_the_op_is_refused_by_name():
    p, _ = program()
    p.add_op(_lib.OP_STORE_SCALAR, io=4, ip=(0,))
    with pytest.raises(NotImplementedError, match="DSP_OP_MULTI_EXTREMA.*get_multi_local_extrema.*LOAD, MULTI_EXTREMA, STORE, STORE, STORE_SCALAR, STORE_SCALAR"):
        plan(p)
    p, _ = program()
    p.ops.insert(1, (_lib.OP_BL_SUBTRACT, 0, 0, 0, (), (Scalar.const(1.0),)))  # an intermediate as the source: rows in memory only
    with pytest.raises(NotImplementedError, match="DSP_OP_MULTI_EXTREMA"):
        plan(p)
    p, _ = program(count_dtype=np.float32)
    with pytest.raises(NotImplementedError, match="DSP_U32"):
        plan(p)
    p, _ = program(dtype=np.float64)
    p.io[0] = p.io[0][:2] + (_lib.F32,) + p.io[0][3:]  # float32 rows in the float64 loop: no kernel of that pair
    with pytest.raises(NotImplementedError, match="float64 loop"):
        plan(p, np.float64)


def test_the_reference_s_checks_and_the_two_refusals():
    with pytest.raises(DSPFatal, match="The length of your return array must be smaller than the length of your waveform"):
        plan(program(n=20, m=20)[0])
    for deltas in ((-1.0, 1.0), (1.0, -1e-30)):
        with pytest.raises(DSPFatal, match="Delta must be positive"):
            plan(program(deltas=deltas)[0])
    plan(program(deltas=(np.nan, 0.0))[0])  # (a NaN delta is the NaN rule's business, zero is allowed)
    for direction in (-1, 4):
        with pytest.raises(DSPFatal, match="search direction type not found."):
            plan(program(direction=direction)[0])
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema: search_direction 2"):
        plan(program(direction=2)[0])
    plan(program(direction=3, m=64)[0])
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema: search_direction 3 takes lists of at most 64"):
        plan(program(direction=3, m=65)[0])
    plan(program(direction=0, m=512)[0])


def test_registry_abi_and_messages():
    from dspeed_amd import processors

    g = processors.get_multi_local_extrema
    assert "get_multi_local_extrema" in processors.__all__
    assert g.signature == "(n),(),(),(),(),(),(m),(m),(),()" and g.types == ["ffffffffII", "ddddddddII"] and (g.nin, g.nout) == (10, 0)
    with pytest.raises(TypeError, match="vt_max_out and vt_min_out must be passed"):
        g(np.zeros(10, np.float32), 1, 1, 0, 0, 0)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "dsp_get_multi_local_extrema_f32") and hasattr(L, "dsp_get_multi_local_extrema_f64")
    assert _lib.OP_MULTI_EXTREMA == 34
    L.dsp_fatal_message.restype = ctypes.c_char_p
    assert [L.dsp_fatal_message(c).decode() for c in (26, 27, 28)] == [
        "The length of your return array must be smaller than the length of your waveform", "Delta must be positive", "search direction type not found."]


def test_a_recipe_stages_the_processor_ahead_of_its_program(monkeypatch):
    """compiled without a device: the processor becomes a stage of its own whose program the planner gives dsp_extrema_kernel; an intermediate
    source is written to rows first, expressions of fit results get small programs of their own; counts are uint32, a computed vector_len is
    an output (a hidden one here); what a recipe cannot have is refused with the processor's name"""
    import extrema_cases as xc

    from dspeed_amd.processing_chain import build_processing_chain

    M = "dspeed.processors"
    g = {x.name: x for x in xc.recipe_groups()}[f"rcppz_n{xc.RECIPE_N}"]
    tb = {"waveform": g.extra["raw"], "baseline": g.extra["baseline"]}
    peaks = lambda src, args, lists: {"function": "get_multi_local_extrema", "module": M,  # noqa: E731
                                      "args": [src, *args, *lists, "n_max_out", "n_min_out"], "unit": ["ns", "ns", "none", "none"]}
    key = "vt_max_out, vt_min_out, n_max_out, n_min_out"
    chain, _, out = build_processing_chain({"outputs": ["vt_max_out"], "processors": {
        key: peaks("waveform", [5, 5, 0, 10, 0], ["vt_max_out(10, vector_len=n_max_out)", "vt_min_out(10)"])}}, tb)
    assert [plan(st["program"])["kernel"] for st in chain._stages if "get_multi_local_extrema" in st["what"]] == ["dsp_extrema_kernel"]
    assert chain.vector_lens == {"vt_max_out": "n_max_out"} and chain.hidden_outputs == ["n_max_out"]
    assert out["vt_max_out"].shape == (xc.RECIPE_ROWS, 10) and out["vt_max_out"].dtype == np.float32 and out["n_max_out"].dtype == np.uint32
    procs = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "baseline", "wf_blsub"]},
             "wf_pz": {"function": "pole_zero", "module": M, "args": ["wf_blsub", xc.RECIPE_TAU, "wf_pz"]},
             "bl_mean, bl_std, bl_slope, bl_intercept": {"function": "linear_slope_fit", "module": M,
                                                         "args": [f"wf_blsub[0:{xc.RECIPE_FIT}]", "bl_mean", "bl_std", "bl_slope", "bl_intercept"]},
             key: peaks("wf_pz", ["5*bl_std", "bl_std", 1, "bl_mean + 3*bl_std", 0], ["vt_max_out(20)", "vt_min_out(20)"])}
    chain, _, out = build_processing_chain({"outputs": ["vt_max_out", "vt_min_out", "n_max_out", "n_min_out"], "processors": procs}, tb)
    kernels = [plan(st["program"])["kernel"] for st in chain._stages]
    assert kernels.count("dsp_extrema_kernel") == 1 and "dsp_pz_rows_kernel" in kernels and kernels.count("dsp_scalar_kernel") >= 2
    assert out["n_max_out"].dtype == np.uint32 and out["n_min_out"].dtype == np.uint32 and chain.hidden_outputs == []
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema.*search_direction 2"):
        build_processing_chain({"outputs": ["n_max_out"], "processors": {key: peaks("waveform", [5, 5, 2, 10, 0], ["vt_max_out(10)", "vt_min_out(10)"])}}, tb)
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema.*at most 64"):
        build_processing_chain({"outputs": ["n_max_out"], "processors": {key: peaks("waveform", [5, 5, 3, 10, 0], ["vt_max_out(65)", "vt_min_out(65)"])}}, tb)
    monkeypatch.setenv("DSPEED_HIP_NO_STAGES", "1")
    with pytest.raises(NotImplementedError, match="get_multi_local_extrema.*DSPEED_HIP_NO_STAGES"):
        build_processing_chain({"outputs": ["n_max_out"], "processors": {key: peaks("waveform", [5, 5, 0, 10, 0], ["vt_max_out(10)", "vt_min_out(10)"])}}, tb)
