"""sort on the device (dsp_sort.hip): every case of tests/sort_cases.py through the gufunc and through a planned chain, compared for
equality with ``np.sort`` and the NaN rule -- values, the multiset of bit patterns, the NaN rows and their clean neighbours, the canaries
between strided rows --, the median and two quantiles of a recipe bit for bit, and one full-size launch."""
import numpy as np
import pytest

import sort_cases as sc

pytestmark = pytest.mark.gpu

M = "dspeed.processors"
POISON = {"f32": -777.0, "f64": -777.0, "i16": -777, "u16": 777}


@pytest.mark.parametrize("rows", list(sc.ROWS))
def test_every_case_through_the_gufunc(rows):
    from dspeed_amd.processors import sort

    book = sc.cases(rows)
    assert {c.count for c in book} == set(sc.ROW_COUNTS) and {c.n for c in book} == {n for n in sc.LENGTHS if n <= sc.limit(rows)}
    for c in book:
        sc.check(c, sort(c.w), "gufunc")
    c = next(c for c in book if c.n == 257 and c.count == 7)
    out = np.full(c.w.shape, -7, dtype=c.loop)
    assert sort(c.w, out) is out  # the output passed
    sc.check(c, out, "gufunc, output passed")
    one = sort(c.w[0])  # a 1-D call
    assert one.shape == (c.n,) and np.array_equal(one, c.want()[0], equal_nan=True)


@pytest.mark.parametrize("rows", list(sc.ROWS))
def test_every_case_through_a_planned_chain_with_canaries(rows):
    """rows n + 3 apart on the way in and n + 5 on the way out, from an element that is not 16-byte aligned for odd n: nothing between the
    rows is written"""
    from dspeed_amd.chain import Chain, plan
    from dspeed_amd.device import DeviceArray

    chain, built_for = None, None
    for c in sc.cases(rows):
        if built_for != c.n:
            if chain is not None:
                chain.close()
            p = sc.program(c.n, sc.ROWS[rows], c.loop, row_stride=c.n + sc.IN_PAD, out_stride=c.n + sc.OUT_PAD)
            assert plan(p, c.loop)["kernel"] == sc.KERNEL
            chain, built_for = Chain(p, compute_dtype=c.loop), c.n
            assert chain.kernel_name == sc.KERNEL
            g = chain.geometry(c.count)
            assert g["blocks"] == (c.count if sc.padded(c.n) > sc.T else (c.count + 3) // 4) and g["waves_per_block"] == 4, (c.name, g)
        d = DeviceArray.from_numpy(c.strided_input(POISON[rows]))
        o = DeviceArray.from_numpy(np.full((c.count, c.n + sc.OUT_PAD), -7, dtype=c.loop))
        chain.execute({"w": d, "out": o}, c.count)
        chain.check()
        got = o.to_numpy()
        sc.check(c, np.ascontiguousarray(got[:, :c.n]), "chain")
        assert (got[:, c.n:] == -7).all(), c.name
        assert d.to_numpy().tobytes() == c.strided_input(POISON[rows]).tobytes(), c.name  # (the rows are read, never written)
        d.free(), o.free()
    chain.close()


def test_rows_and_output_on_the_device():
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import sort

    for rows, n in (("f32", 257), ("f64", 4097), ("u16", 65)):
        c = next(c for c in sc.cases(rows) if c.n == n and c.count == 5)
        d, do = DeviceArray.from_numpy(c.w), DeviceArray(c.w.shape, c.loop)
        assert sort(d, do) is do
        sc.check(c, do.to_numpy(), "device arrays")
        d.free(), do.free()


def test_the_refusals():
    from dspeed_amd.processors import sort

    with pytest.raises(NotImplementedError, match="sort: the float64 loop takes float64 rows on the device"):
        sort(np.zeros((4, 10), np.int32))
    with pytest.raises(NotImplementedError, match=f"sort: {sc.LIMITS} \\(16385 given\\)"):
        sort(np.zeros((1, 16385), np.float32))
    with pytest.raises(NotImplementedError, match=f"sort: {sc.LIMITS} \\(8193 given\\)"):
        sort(np.zeros((1, 8193), np.float64))


def _table(rng, rows=12, n=1000):
    from dspeed_amd.processing_chain import WaveformInput

    w = (10000 + rng.integers(-20, 21, (rows, n)) + (np.arange(n) >= 600) * rng.integers(500, 5000, (rows, 1))).astype(np.uint16)
    return w, {"waveform": WaveformInput(w, 16.0), "bl": rng.uniform(9990, 10010, rows).astype(np.float32)}


def _pick(name, source, at):
    return {name: {"function": "fixed_time_pickoff", "module": M, "args": [source, at, "'i'", name]}}


def test_median_and_quantiles_of_a_recipe_on_uint16_rows():
    from dspeed_amd.processing_chain import build_processing_chain

    w, tb = _table(np.random.default_rng(11))
    procs = {"wf_sorted": {"function": "sort", "module": M, "args": ["waveform", "wf_sorted"]}}
    procs.update(_pick("med", "wf_sorted", "len(wf_sorted)/2"))
    procs.update(_pick("q10", "wf_sorted", "0.1*len(wf_sorted)"))
    procs.update(_pick("q90", "wf_sorted", "0.9*len(wf_sorted)"))
    want = np.sort(w.astype(np.float32), axis=1)
    for outputs in (["med", "q10", "q90"], ["med", "q10", "q90", "wf_sorted"]):
        chain, _, out = build_processing_chain({"outputs": outputs, "processors": procs}, tb)
        chain.execute()
        assert [k for _w, k in chain.kernels()].count(sc.KERNEL) == 1
        for name, at in (("med", 500), ("q10", 100), ("q90", 900)):
            assert out[name].dtype == np.float32 and np.array_equal(out[name].view(np.uint32), want[:, at].view(np.uint32)), name
        if "wf_sorted" in outputs:
            assert out["wf_sorted"].dtype == np.float32 and np.array_equal(out["wf_sorted"], want)


def test_a_waveform_the_program_computes_is_written_to_memory_and_sorted():
    from dspeed_amd.processing_chain import build_processing_chain

    w, tb = _table(np.random.default_rng(12))
    procs = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]},
             "wf_sorted": {"function": "sort", "module": f"{M}.sort", "args": ["wf_blsub", "wf_sorted"]}}
    procs.update(_pick("med", "wf_sorted", "len(wf_sorted)/2"))
    chain, _, out = build_processing_chain({"outputs": ["med", "wf_sorted"], "processors": procs}, tb)
    chain.execute()
    whats = [what for what, _k in chain.kernels()]
    assert any("wf_blsub -> HBM" in x for x in whats) and [k for _w, k in chain.kernels()].count(sc.KERNEL) == 1
    want = np.sort(w.astype(np.float32) - tb["bl"][:, None], axis=1)
    assert np.array_equal(out["wf_sorted"], want) and np.array_equal(out["med"], want[:, 500])


def test_one_full_size_launch():
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import sort

    rng = np.random.default_rng(13)
    w = rng.standard_normal((4096, 8192), dtype=np.float32)
    w[::97, ::89] = np.inf
    w[5::101, 3::83] = -0.0
    d, do = DeviceArray.from_numpy(w), DeviceArray(w.shape, np.float32)
    assert sort(d, do) is do
    got = do.to_numpy()
    d.free(), do.free()
    w.sort(axis=1)
    assert np.array_equal(got, w)
