"""psd and fft on the device (dsp_spectrum.hip), every group of tests/spectrum_cases.py held to its rules: exact bins on the power-of-two
rows that multiply only zeros by inexact twiddles, the error cap against NumPy's float64 rfft on every finite row, psd against the device's
own fft, the bar against the reference's float32 error on noise rows (tests/golden/spectrum.npz), NaN bins for rows with a NaN or an
infinity -- through the gufuncs, the C entries and a chain run twice."""
import ctypes as C

import numpy as np
import pytest

import golden_util
import spectrum_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def book():
    return {c.name: c for c in golden_util.cases(sc.BOOK, kernel=sc.KERNEL)}


@pytest.fixture(scope="module")
def groups():
    return sc.groups()


def _complex(loop):
    return np.complex64 if loop is np.float32 else np.complex128


def test_every_group_through_the_gufuncs(book, groups):
    from dspeed_amd.processors import fft, psd

    assert any(len(g.w) % 4 for g in groups if not sc.wide(g.n, g.loop))  # a partial workgroup among the launches
    for g in groups:
        m = g.n // 2 + 1
        X, P = np.full((len(g.w), m), -7, dtype=_complex(g.loop)), np.full((len(g.w), m), -7, dtype=g.loop)
        assert fft(g.w, X) is X and psd(g.w, P) is P
        figures = sc.check_group(g, book[g.name], X, P, "gufunc")
        print(g.name, {k: (round(a, 3), None if b is None else round(b, 2)) for k, (a, b) in figures.items()})


def test_every_group_through_the_c_entries(book, groups):
    """device-resident rows and outputs; the rows once more from an odd element on, a stride longer than the row, and outputs apart"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray

    L, row = _lib.lib(), C.c_int64(-1)
    for g in groups:
        n, m, R = g.n, g.n // 2 + 1, len(g.w)
        code = {"f32": _lib.F32, "f64": _lib.F64, "i16": _lib.I16, "u16": _lib.U16}[g.rows]
        loop = _lib.F32 if g.loop is np.float32 else _lib.F64
        d = DeviceArray.from_numpy(g.w)
        dX, dP = DeviceArray((R, m), _complex(g.loop)), DeviceArray((R, m), g.loop)
        assert L.dsp_fft(d.ptr, code, R, n, n, loop, dX.ptr, m, 2 * m, None, C.byref(row)) == 0, _lib.last_error()
        assert L.dsp_psd(d.ptr, code, R, n, n, loop, dP.ptr, m, m, None, C.byref(row)) == 0, _lib.last_error()
        X, P = dX.to_numpy(), dP.to_numpy()
        sc.check_group(g, book[g.name], X, P, "C entry")
        if g.n not in (1, 65, 1000, 1024, 4096):
            continue
        # an unaligned start (one element in), rows n + 3 apart, outputs m + 2 bins apart: the same bits
        stride = n + 3
        block = np.zeros(R * stride + 1, dtype=g.w.dtype)
        for r in range(R):
            block[1 + r * stride: 1 + r * stride + n] = g.w[r]
        d2 = DeviceArray.from_numpy(block)
        dX2 = DeviceArray.from_numpy(np.full((R, m + 2), -7, dtype=_complex(g.loop)))
        dP2 = DeviceArray.from_numpy(np.full((R, m + 2), -7, dtype=g.loop))
        at = d2.ptr + g.w.dtype.itemsize
        assert L.dsp_fft(at, code, R, n, stride, loop, dX2.ptr, m, 2 * (m + 2), None, C.byref(row)) == 0, _lib.last_error()
        assert L.dsp_psd(at, code, R, n, stride, loop, dP2.ptr, m, m + 2, None, C.byref(row)) == 0, _lib.last_error()
        X2, P2 = dX2.to_numpy(), dP2.to_numpy()
        assert np.array_equal(X2[:, :m].view(g.loop), X.view(g.loop), equal_nan=True) and np.array_equal(P2[:, :m], P, equal_nan=True), g.name
        assert (X2[:, m:] == -7).all() and (P2[:, m:] == -7).all(), g.name


def test_one_row_and_outputs_on_the_device(book, groups):
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import fft, psd

    for name in ("f32_n1000", "f64_n1024", "u16_n65"):
        g = next(g for g in groups if g.name == name)
        m = g.n // 2 + 1
        X, P = np.empty((len(g.w), m), dtype=_complex(g.loop)), np.empty((len(g.w), m), dtype=g.loop)
        fft(g.w, X), psd(g.w, P)
        x1, p1 = np.empty(m, dtype=X.dtype), np.empty(m, dtype=P.dtype)  # a 1-D call
        assert fft(g.w[2], x1) is x1 and psd(g.w[2], p1) is p1
        assert np.array_equal(x1, X[2]) and np.array_equal(p1, P[2])
        d, dX, dP = DeviceArray.from_numpy(g.w), DeviceArray((len(g.w), m), X.dtype), DeviceArray((len(g.w), m), P.dtype)
        assert fft(d, dX) is dX and psd(d, dP) is dP
        assert np.array_equal(dX.to_numpy().view(g.loop), X.view(g.loop), equal_nan=True) and np.array_equal(dP.to_numpy(), P, equal_nan=True)


@pytest.mark.parametrize("n", [1024, 1000, 16384])
def test_one_chain_executed_twice_gives_identical_bits(groups, n):
    """the tables are the chain's, written when it is created: a second launch finds them as the first did"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray

    g = next(g for g in groups if g.name == f"f32_n{n}")
    m = n // 2 + 1
    chain = Chain(sc.program(n, "fft"))
    assert chain.kernel_name == "dsp_spectrum_kernel"
    d = DeviceArray.from_numpy(g.w)
    outs = [DeviceArray.from_numpy(np.full((len(g.w), 2 * m), -7, dtype=np.float32)) for _ in range(2)]
    for o in outs:
        chain.execute({"w": d, "out": o}, len(g.w))
        chain.check()
    a, b = (o.to_numpy() for o in outs)
    assert np.array_equal(a, b, equal_nan=True) and not (a == -7).any()
    X = np.ascontiguousarray(a).view(np.complex64)
    X64, finite = g.truth(), g.finite()
    for r in np.flatnonzero(finite):
        assert sc.rel_l2(X[r], X64[r]) <= sc.cap(n, np.float32)
    chain.close()


def test_the_reference_s_check_and_the_refusals():
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import fft, psd

    w = np.arange(40, dtype=np.float32).reshape(4, 10)
    with pytest.raises(DSPFatal, match="Size of psd must be len\\(w_in\\)//2\\+1 = 6"):
        psd(w, np.empty((4, 5), np.float32))
    with pytest.raises(DSPFatal, match="Size of fft must be len\\(w_in\\)//2\\+1 = 6"):
        fft(w, np.empty((4, 7), np.complex64))
    with pytest.raises(TypeError, match="psd\\(w_in, psd_out\\): psd_out must be passed \\(len\\(w_in\\)//2 \\+ 1 bins\\)"):
        psd(w)
    with pytest.raises(NotImplementedError, match="psd: the float64 loop takes float64 rows on the device"):
        psd(w.astype(np.int32), np.empty((4, 6), np.float64))
    with pytest.raises(NotImplementedError, match="fft: the float32 loop takes rows of a power of two up to 16384 samples and of any other length up to 4096 \\(4097 given\\)"):
        fft(np.zeros((1, 4097), np.float32), np.empty((1, 2049), np.complex64))
    with pytest.raises(NotImplementedError, match="psd: the float64 loop takes rows of a power of two up to 8192 samples and of any other length up to 2048 \\(16384 given\\)"):
        psd(np.zeros((1, 16384), np.float64), np.empty((1, 8193), np.float64))


def test_psd_in_a_recipe_on_uint16_rows():
    """a slice of the input rows and a waveform the program computes (written to memory first) as sources: the spectrum is the gufunc's on
    the same rows bit for bit, and an op of the program reads it"""
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain
    from dspeed_amd.processors import psd

    M = "dspeed.processors"
    rng = np.random.default_rng(11)
    w = (10000 + rng.integers(-20, 21, (13, 4096)) + (np.arange(4096) >= 1500) * rng.integers(500, 5000, (13, 1))).astype(np.uint16)
    bl = rng.uniform(9990, 10010, 13).astype(np.float32)
    amax = {"function": "amax", "module": "numpy", "args": ["psd_out[1:]", 1, "p_max"], "kwargs": {"signature": "(n),()->()", "types": ["fi->f"]}}
    blsub = {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]}
    for source, rows, first in (("waveform[96:3096]", w[:, 96:3096], {}),
                                ("wf_blsub", w.astype(np.float32) - bl[:, None], {"wf_blsub": blsub}),
                                ("wf_blsub[:3000]", (w.astype(np.float32) - bl[:, None])[:, :3000], {"wf_blsub": blsub})):
        n = rows.shape[1]
        decl = f"psd_out({n // 2 + 1})" if "[" in source else "psd_out(len(wf_blsub)//2+1, period=1/wf_blsub.period/len(wf_blsub))"
        procs = dict(first, psd_out={"function": "psd", "module": f"{M}.fft", "args": [source, decl]}, p_max=amax)
        chain, _, out = build_processing_chain({"outputs": ["psd_out", "p_max"], "processors": procs}, {"waveform": WaveformInput(w, 16.0), "bl": bl})
        chain.execute()
        assert [k for _w, k in chain.kernels()].count("dsp_spectrum_kernel") == 1
        want = np.empty((13, n // 2 + 1), dtype=np.float32)
        psd(np.ascontiguousarray(rows), want)
        assert np.isfinite(want).all() and np.array_equal(out["psd_out"], want), source
        assert np.array_equal(out["p_max"], want[:, 1:].max(axis=1)), source


def test_the_geometry_by_length():
    from dspeed_amd.chain import Chain

    for n, loop in ((2048, np.float32), (4096, np.float32), (511, np.float32), (513, np.float32), (1024, np.float64), (2048, np.float64)):
        chain = Chain(sc.program(n, "psd", loop, loop), compute_dtype=loop)
        g = chain.geometry(10)
        assert g["blocks"] == (10 if sc.wide(n, loop) else 3) and g["waves_per_block"] == 4, (n, g)
        chain.close()
