"""interpolating_upsampler on the device (dsp_interp.hip): the whole book of tests/interp_cases.py through the C entry -- every row type,
loop and mode, output rows at element offsets 0 .. 3 of a 16-byte boundary with a sentinel before, between and behind them --, through the
gufunc (host arrays and DeviceArrays) and through the recipe stage, compared with ``np.array_equal`` against the emulation of numba's typing,
NaN positions included.  Exact equality holds for mode 's' too: a warm-up of 48 samples puts a perturbation of 3e-28 of the row's scale
ahead of the same operations (pickoff_spline's argument)."""
import numpy as np
import pytest

import interp_cases as ic

pytestmark = pytest.mark.gpu

M = "dspeed.processors"
SENTINEL = -7.0
CODES = {"f32": "F32", "i16": "I16", "u16": "U16", "f64": "F64"}


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(want))


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    r, c = np.nonzero(bad)
    return len(r), sorted(set(r.tolist()))[:6], c[:6].tolist(), got[bad][:4], want[bad][:4]


@pytest.mark.parametrize("rows", list(ic.ROWS))
def test_the_whole_book_through_the_c_entry_with_sentinels(rows):
    """rows n or n + 3 apart on the way in; on the way out m + 0 .. 2 apart from an element 0 .. 3 past a 16-byte boundary: 16-byte stores
    where start and stride allow, a sample per lane otherwise, and nothing but the m samples of every row written -- not the store at m
    the reference's mode 's' begins with, not a tail lane's"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.gufunc import run

    fn = _lib.lib().dsp_interp_upsample_rows
    loop = ic.LOOPS[rows]
    esz, loop_code, code = np.dtype(loop).itemsize, _lib.F32 if loop is np.float32 else _lib.F64, getattr(_lib, CODES[rows])
    vectors = set()
    for k, (n, m) in enumerate(ic.pairs(rows)):
        w = ic.rows_of(rows, n)
        R = len(w)
        in_stride = n + (3 if k % 2 else 0)
        block = np.full((R, in_stride), 77, dtype=w.dtype)
        block[:, :n] = w
        off, out_stride = k % 4, m + k % 3
        total = 4 + R * out_stride + 8
        blank = np.full(total, SENTINEL, dtype=loop)
        d, o = DeviceArray.from_numpy(block), DeviceArray.from_numpy(blank)
        assert o.ptr % 16 == 0
        vectors.add(off == 0 and (out_stride * esz) % 16 == 0)
        for mode in ic.modes_for(rows, n, m):
            o.copy_from(blank)
            run(fn, "interpolating_upsampler", d.ptr, code, R, n, in_stride, loop_code, ord(mode), o.ptr + off * esz, m, out_stride)
            got = o.to_numpy()
            body = got[off:off + R * out_stride].reshape(R, out_stride)
            want = ic.want(rows, n, m, mode)
            assert _same(np.ascontiguousarray(body[:, :m]), want), (rows, n, m, mode, _diff(body[:, :m], want))
            assert (got[:off] == SENTINEL).all() and (body[:, m:] == SENTINEL).all() and (got[off + R * out_stride:] == SENTINEL).all(), (rows, n, m, mode)
        assert d.to_numpy().tobytes() == block.tobytes()  # (the rows are read, never written)
        d.free(), o.free()
    assert vectors == {True, False}


@pytest.mark.parametrize("rows", list(ic.ROWS))
def test_the_gufunc_on_host_arrays_and_device_arrays(rows):
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import interpolating_upsampler

    loop = ic.LOOPS[rows]
    for n, m in ic.pairs(rows)[::6] + ic.NAMED_PAIRS:
        w = ic.rows_of(rows, n)
        for mode in ic.modes_for(rows, n, m):
            want = ic.want(rows, n, m, mode)
            out = np.full((len(w), m), SENTINEL, dtype=loop)
            assert interpolating_upsampler(w, mode, out) is out
            assert _same(out, want), (rows, n, m, mode, _diff(out, want))
            d, do = DeviceArray.from_numpy(np.ascontiguousarray(w)), DeviceArray((len(w), m), loop)
            assert interpolating_upsampler(d, ord(mode), do) is do
            assert _same(do.to_numpy(), want), (rows, n, m, mode)
            d.free(), do.free()
    w = ic.rows_of(rows, 17)
    one = np.empty(34, dtype=loop)
    interpolating_upsampler(w[1], np.int8(ord("l")), one)  # a 1-D call, the mode as the reference passes it
    assert _same(one, ic.want(rows, 17, 34, "l")[1])


def test_more_rows_than_a_workgroup_and_than_a_wave_of_workgroups():
    """4099 rows: workgroups of four rows and a remainder, in both geometries"""
    from dspeed_amd.processors import interpolating_upsampler

    for n, m, mode in ((50, 500, "s"), (50, 117, "h"), (2049, 2050, "l"), (683, 684, "s")):
        base = ic.rows_of("f32", n)
        count = 4099 if n < 100 else 41
        w = np.ascontiguousarray(np.tile(base, (count // len(base) + 1, 1))[:count])
        want = np.tile(ic.want("f32", n, m, mode), (count // len(base) + 1, 1))[:count]
        out = np.empty((count, m), np.float32)
        interpolating_upsampler(w, mode, out)
        assert _same(out, want), (n, m, mode, _diff(out, want))


def test_the_launch_geometry_on_both_sides_of_the_switch():
    """a wavefront per row, four rows to a workgroup, while a row fills at most 8 KiB of LDS; a workgroup per row above"""
    from dspeed_amd.chain import Chain

    for n, mode, count, blocks in ((2048, "l", 7, 2), (2049, "l", 7, 7), (682, "s", 5, 2), (683, "s", 5, 5)):
        chain = Chain(ic.program(n, 2 * n, mode), compute_dtype=np.float32)
        g = chain.geometry(count)
        assert chain.kernel_name == ic.KERNEL and g["blocks"] == blocks and g["waves_per_block"] == 4, (n, mode, g)
        chain.close()


def test_the_refusals():
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import interpolating_upsampler as up

    with pytest.raises(NotImplementedError, match=f"interpolating_upsampler: {ic.LIMITS} \\(16385 given\\): a row lives in 64 KiB of LDS"):
        up(np.zeros((1, 16385), np.float32), "l", np.zeros((1, 10), np.float32))
    with pytest.raises(NotImplementedError, match=f"interpolating_upsampler: {ic.SPLINE_LIMITS} \\(5457 given\\)"):
        up(np.zeros((1, 5457), np.float32), "s", np.zeros((1, 10), np.float32))
    with pytest.raises(NotImplementedError, match="mode 'h' takes rows of at least 2 samples \\(1 given\\)"):
        up(np.zeros((3, 1), np.float32), "h", np.zeros((3, 10), np.float32))
    with pytest.raises(DSPFatal, match="Unrecognized interpolation mode"):
        up(np.zeros((3, 8), np.float32), "x", np.zeros((3, 16), np.float32))
    with pytest.raises(DSPFatal, match="integer multiple of len\\(w_in\\) for mode 'i'"):
        up(np.zeros((3, 8), np.float32), "i", np.zeros((3, 20), np.float32))
    with pytest.raises(TypeError, match="w_out must be passed"):
        up(np.zeros((3, 8), np.float32), "l")


def _table(rng, rows=12, n=100):
    from dspeed_amd.processing_chain import WaveformInput

    w = (10000 + rng.integers(-20, 21, (rows, n)) + (np.arange(n) >= 60) * rng.integers(500, 5000, (rows, 1))).astype(np.uint16)
    return w, {"waveform": WaveformInput(w, 16.0), "bl": rng.uniform(9990, 10010, rows).astype(np.float32)}


def _recipe(mode, source="waveform", first=None, factor=10):
    """the reference's docstring example (upsampler.py:91-102), min_max and time_point_thresh of the upsampled row behind it"""
    procs = dict(first or {})
    procs["wf_up"] = {"function": "interpolating_upsampler", "module": M,
                      "args": [source, f"'{mode}'", f"wf_up(len({source})*{factor}, period={source}.period/{factor})"]}
    procs["tp_min, tp_max, wf_min, wf_max"] = {"function": "min_max", "module": M, "args": ["wf_up", "tp_min", "tp_max", "wf_min", "wf_max"]}
    procs["tp_50"] = {"function": "time_point_thresh", "module": M, "args": ["wf_up", "0.5*(wf_max+wf_min)", "tp_max", 0, "tp_50"]}
    return procs


def _tp_50(x, thr, start):
    """time_point_thresh walking backward from `start` (time_point_thresh.py:80-92), in samples of the finer grid"""
    out = np.full(len(x), np.nan, np.float32)
    for r in range(len(x)):
        for i in range(int(start[r]), 0, -1):
            if (x[r, i - 1] < thr[r] <= x[r, i]) or (x[r, i - 1] > thr[r] >= x[r, i]):
                out[r] = i
                break
    return out


@pytest.mark.parametrize("mode", list("slh"))
def test_the_docstring_recipe_end_to_end(mode):
    from dspeed_amd.processing_chain import build_processing_chain

    w, tb = _table(np.random.default_rng(21))
    chain, _, out = build_processing_chain({"outputs": ["wf_up", "wf_max", "wf_min", "tp_max", "tp_50"], "processors": _recipe(mode)}, tb)
    chain.execute()
    assert [k for _w, k in chain.kernels()].count(ic.KERNEL) == 1
    want = ic.emulate(w.astype(np.float32), mode, 1000)
    assert out["wf_up"].dtype == np.float32 and _same(out["wf_up"], want), _diff(out["wf_up"], want)
    assert np.array_equal(out["wf_max"], want.max(axis=1)) and np.array_equal(out["wf_min"], want.min(axis=1))
    # times without a unit are samples of the finer grid
    t_max = want.argmax(axis=1)
    thr = (np.float32(0.5) * (want.max(axis=1) + want.min(axis=1))).astype(np.float32)
    assert np.array_equal(out["tp_max"], t_max.astype(np.float32)) and np.array_equal(out["tp_50"], _tp_50(want, thr, t_max))
    assert not np.isnan(out["tp_50"]).any()


def test_a_waveform_the_program_computes_is_written_to_memory_and_resampled():
    from dspeed_amd.processing_chain import build_processing_chain

    w, tb = _table(np.random.default_rng(22))
    blsub = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]}}
    procs = _recipe("l", "wf_blsub", blsub, factor=3)
    procs["wf_up"]["module"] = f"{M}.upsampler"
    chain, _, out = build_processing_chain({"outputs": ["wf_up", "wf_max"], "processors": procs}, tb)
    chain.execute()
    whats = [what for what, _k in chain.kernels()]
    assert any("wf_blsub -> HBM" in x for x in whats) and [k for _w, k in chain.kernels()].count(ic.KERNEL) == 1
    want = ic.emulate(w.astype(np.float32) - tb["bl"][:, None], "l", 300)
    assert _same(out["wf_up"], want) and np.array_equal(out["wf_max"], want.max(axis=1))
