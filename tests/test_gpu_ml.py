"""The neural-network layers on the device (dsp_dense.hip): the book of tests/ml_cases.py through the C entries -- every row type and loop,
padded row strides and odd lengths (the scalar loader), every n and m at which the kernel takes another path, partial row tiles, with a
sentinel behind every output row --, through the gufuncs and through the recipe stages.

In the float32 loop 'r' and 'l' equal the emulation (one fmaf chain per output in ascending k, the bias, numba's typing) in every bit; every
activation in both loops stays within the bound of ``ml_cases.bound`` of the reference body evaluated one precision up."""
import numpy as np
import pytest

import ml_cases as mc

pytestmark = pytest.mark.gpu

M = "dspeed.processors"
SENTINEL = -7.0
CODES = {"f32": "F32", "i16": "I16", "u16": "U16", "f64": "F64"}


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    idx = np.argwhere(bad)
    return len(idx), idx[:4].tolist(), got[bad][:4], want[bad][:4]


def _dense(fn, d_rows, code, count, n, in_stride, loop_code, wd, bd, act, o, off, esz, m, out_stride):
    from dspeed_amd.gufunc import run

    run(fn, "dense_layer", d_rows.ptr, code, count, n, in_stride, loop_code, wd.ptr, bd.ptr if bd is not None else None, ord(act), o.ptr + off * esz, m, out_stride)


@pytest.mark.parametrize("rows", list(mc.ROWS))
def test_the_whole_book_through_the_c_entry_with_sentinels(rows):
    """rows n or n + 3 apart on the way in (the 16-byte loader where stride and length allow, the scalar one elsewhere), m + 0 .. 2 apart on the
    way out from an element 0 .. 3 past the buffer's start; nothing but the m values of every row written"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray

    fn = _lib.lib().dsp_dense_rows
    loop = mc.LOOPS[rows]
    esz, loop_code, code = np.dtype(loop).itemsize, _lib.F32 if loop is np.float32 else _lib.F64, getattr(_lib, CODES[rows])
    worst, vectors = 0.0, set()
    for k, (n, m, count) in enumerate(mc.shapes(rows)):
        act, with_bias = mc.variant(k)
        x = mc.rows_of(rows, count, n)
        w, b, _mu, _var = mc.layer_of(rows, n, m)
        in_stride = n + (3 if k % 2 else 0)
        block = np.full((count, in_stride), 77, dtype=x.dtype)
        block[:, :n] = x
        off, out_stride = k % 4, m + k % 3
        blank = np.full(4 + count * out_stride + 8, SENTINEL, dtype=loop)
        d, o, wd = DeviceArray.from_numpy(block), DeviceArray.from_numpy(blank), DeviceArray.from_numpy(w)
        bd = DeviceArray.from_numpy(b) if with_bias else None
        vectors.add((in_stride * x.dtype.itemsize) % 16 == 0 and (n * x.dtype.itemsize) % 16 == 0)
        _dense(fn, d, code, count, n, in_stride, loop_code, wd, bd, act, o, off, esz, m, out_stride)
        got = o.to_numpy()
        body = got[off:off + count * out_stride].reshape(count, out_stride)
        res = np.ascontiguousarray(body[:, :m])
        assert (got[:off] == SENTINEL).all() and (body[:, m:] == SENTINEL).all() and (got[off + count * out_stride:] == SENTINEL).all(), (rows, n, m, count)
        if loop is np.float32 and act in "rl":
            want = mc.want(rows, n, m, count, act, with_bias)
            assert _same(res, want), (rows, n, m, count, act, _diff(res, want))
        ok, ratio = mc.within(res, x, w, b if with_bias else None, act)
        worst = max(worst, ratio)
        assert ok, (rows, n, m, count, act, ratio)
        assert d.to_numpy().tobytes() == block.tobytes()  # (the rows are read, never written)
        for a in (d, o, wd, bd):
            if a is not None:
                a.free()
    print(f"{rows}: worst |device - exact| / bound = {worst:.3f}")
    assert vectors == {True, False}


@pytest.mark.parametrize("rows", ["f32", "f64"])
def test_every_activation_and_an_unknown_one_with_and_without_bias(rows):
    from dspeed_amd.processors import classification_layer_no_bias, classification_layer_with_bias, dense_layer_no_bias, dense_layer_with_bias

    loop = mc.LOOPS[rows]
    c = mc.chunk(loop)
    for n, m, count in ((c + 1, 17, 65), (5, 33, 17)):
        x = mc.rows_of(rows, count, n)
        w, b, _mu, _var = mc.layer_of(rows, n, m)
        for act in mc.ACTIVATIONS + mc.UNKNOWN:
            for with_bias in (False, True):
                got = dense_layer_with_bias(x, w, b, act) if with_bias else dense_layer_no_bias(x, w, act)
                one = classification_layer_with_bias(x, w[:, 0], b[0], act) if with_bias else classification_layer_no_bias(x, w[:, 0], act)
                assert got.dtype == loop and got.shape == (count, m) and one.dtype == loop and one.shape == (count,)
                if act == mc.UNKNOWN:
                    assert np.isnan(got).all() and np.isnan(one).all()  # (the reference leaves the NaNs it starts with, without raising)
                    continue
                if loop is np.float32 and act in "rl":
                    assert _same(got, mc.want(rows, n, m, count, act, with_bias)), (n, m, act, with_bias)
                    assert _same(one, mc.want(rows, n, m, count, act, with_bias, classify=True)), (n, m, act, with_bias)
                assert mc.within(got, x, w, b if with_bias else None, act)[0], (n, m, act, with_bias)
                assert mc.within(one, x, w[:, 0], b[0] if with_bias else None, act)[0], (n, m, act, with_bias)
                assert np.array_equal(one, got[:, 0], equal_nan=True)  # (the classification layer is the m = 1 case: the same chain)


def test_the_float64_loop_and_an_fma_chain():
    """reported, and held: v_mfma_f64_16x16x4_f64 is an fma chain in ascending k too"""
    from dspeed_amd.processors import dense_layer_with_bias

    for n, m, count in ((33, 17, 65), (65, 33, 16)):
        x = mc.rows_of("f64", count, n)
        w, b, _mu, _var = mc.layer_of("f64", n, m)
        got = dense_layer_with_bias(x, w, b, "r")
        want = mc.want("f64", n, m, count, "r", True)
        print("float64 loop equals an fma chain:", _same(got, want), _diff(got, want)[0])
        assert _same(got, want), _diff(got, want)


def test_nan_rows_infinities_and_nan_weights():
    from dspeed_amd.processors import classification_layer_no_bias, dense_layer_no_bias, dense_layer_with_bias

    for rows in ("f32", "f64"):
        T = mc.LOOPS[rows]
        n, m, count = mc.chunk(T) + 3, 17, 20
        x = mc.rows_of(rows, count, n).copy()
        w, b, _mu, _var = (a.copy() for a in mc.layer_of(rows, n, m))
        x[3, 0], x[7, n - 1], x[11, n // 2] = np.nan, np.nan, np.nan
        for act in "rlsmt":
            got = dense_layer_with_bias(x, w, b, act)
            assert np.isnan(got[[3, 7, 11]]).all() and not np.isnan(np.delete(got, [3, 7, 11], axis=0)).any(), (rows, act)
        # a NaN against weights of 0: NaN x 0 is NaN, the row comes out NaN through the products, no scan
        zero = np.zeros_like(w)
        for act in "rlsmt":
            got = dense_layer_no_bias(x, zero, act)
            assert np.isnan(got[[3, 7, 11]]).all() and not np.isnan(np.delete(got, [3, 7, 11], axis=0)).any(), (rows, act)
        assert np.isnan(classification_layer_no_bias(x, zero[:, 0], "r")[[3, 7, 11]]).all()
        # infinities are ordinary values of np.dot: inf x positive weights is inf, inf x 0 is NaN, inf - inf is NaN
        y = mc.rows_of(rows, count, n).copy()
        y[2, 1], y[4, 2], y[5, 1], y[5, 2] = np.inf, -np.inf, np.inf, np.inf
        wp = np.abs(w) + T(0.5)
        got = dense_layer_no_bias(y, wp, "l")
        # leaky_relu(+-inf) = inf * 1 + 0.01 * inf * 0: NaN
        assert np.isnan(got[2]).all() and np.isnan(got[4]).all() and np.isnan(got[5]).all()
        got = dense_layer_no_bias(y, wp, "t")
        assert (got[2] == 1).all() and (got[4] == -1).all() and (got[5] == 1).all() and np.isfinite(np.delete(got, [2, 4, 5], axis=0)).all()
        wm = wp.copy()
        wm[2] = -wm[2]
        assert np.isnan(dense_layer_no_bias(y, wm, "t")[5]).all()  # inf - inf
        assert np.isnan(dense_layer_no_bias(y, zero, "t")[[2, 4, 5]]).all()  # inf x 0
        # a NaN among the weights: the columns that hold it, in every row
        w[5, 3] = np.nan
        got = dense_layer_with_bias(mc.rows_of(rows, count, n), w, b, "s")
        assert np.isnan(got[:, 3]).all() and not np.isnan(np.delete(got, 3, axis=1)).any()


def test_the_expressions_as_written():
    """relu of a negative value is -0.0 and relu(-inf) NaN; leaky_relu(+-inf) NaN; in the float32 loop softmax(89) is inf (exp overflows in
    float32) and sigmoid(-100) is 0"""
    from dspeed_amd.processors import classification_layer_no_bias as layer

    one = np.ones(1, np.float32)
    x = np.array([[-3.0], [2.0], [-np.inf], [np.inf], [89.0], [-100.0], [0.0], [-0.0]], np.float32)
    r = layer(x, one, "r")
    assert r[0] == 0 and np.signbit(r[0]) and r[1] == 2 and np.isnan(r[2]) and r[3] == np.inf and r[6] == 0 and not np.signbit(r[6])
    lk = layer(x, one, "l")
    assert np.isnan(lk[2]) and np.isnan(lk[3]) and lk[1] == 2 and lk[0] == np.float32(0.01 * -3.0)
    assert _same(lk, mc.emulate(x, one, None, "l")) and _same(r, mc.emulate(x, one, None, "r"))
    sm = layer(x, one, "m")
    assert sm[4] == np.inf and sm[3] == np.inf and sm[2] == 0 and abs(sm[1] - np.log1p(np.exp(2.0))) < 1e-6
    sg = layer(x, one, "s")
    assert sg[5] == 0 and sg[2] == 0 and sg[3] == 1 and sg[6] == 0.5
    x64 = x.astype(np.float64)
    assert np.isfinite(layer(x64, np.ones(1), "m")[4]) and layer(x64, np.ones(1), "s")[5] > 0  # (the float64 loop: exp(89) and exp(100) are finite)
    t = layer(x, one, "t")
    assert t[2] == -1 and t[3] == 1 and t[6] == 0


@pytest.mark.parametrize("rows", list(mc.ROWS))
def test_fused_and_standalone_normalisation_bit_for_bit(rows):
    """normalisation_layer on its own, then the dense layer on its rows, against LOAD, NORMALISE, DENSE, STORE in one launch"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import dense_layer_with_bias, normalisation_layer

    loop = mc.LOOPS[rows]
    c = mc.chunk(loop)
    for n, m, count in ((c + 5, 17, 65), (2 * c, 16, 130), (3, 1, 5)):
        x = mc.rows_of(rows, count, n)
        w, b, mu, var = mc.layer_of(rows, n, m)
        normed = normalisation_layer(x, mu, var)
        assert normed.dtype == loop and _same(normed, mc.normalise(x.astype(loop), mu, var)), (rows, n)
        apart = dense_layer_with_bias(normed, w, b, "l")
        chain = Chain(mc.program(n, m, "l", norm=True, rows=x.dtype.type, loop=loop), compute_dtype=loop)
        assert chain.kernel_name == mc.KERNEL
        bufs = {k: DeviceArray.from_numpy(np.ascontiguousarray(v)) for k, v in (("in", x), ("means", mu), ("variances", var), ("kernel", w), ("bias", b))}
        bufs["out"] = DeviceArray((count, m), loop)
        chain.execute(bufs, count)
        chain.check()
        fused = bufs["out"].to_numpy()
        chain.close()
        for a in bufs.values():
            a.free()
        assert _same(fused, apart), (rows, n, m, _diff(fused, apart))
        if loop is np.float32:
            assert _same(fused, mc.want(rows, n, m, count, "l", True, normalised=True))


def test_the_limits_and_the_launch_geometry():
    from dspeed_amd.chain import Chain
    from dspeed_amd.processors import dense_layer_no_bias, normalisation_layer

    with pytest.raises(NotImplementedError, match=f"dense_layer_no_bias: {mc.LIMITS} \\(n = 16385, m = 2 given\\)"):
        dense_layer_no_bias(np.zeros((1, 16385), np.float32), np.zeros((16385, 2), np.float32), "r")
    with pytest.raises(NotImplementedError, match=f"dense_layer_no_bias: {mc.LIMITS} \\(n = 4, m = 257 given\\)"):
        dense_layer_no_bias(np.zeros((1, 4), np.float32), np.zeros((4, 257), np.float32), "r")
    with pytest.raises(NotImplementedError, match=f"normalisation_layer: {mc.LIMITS}"):
        normalisation_layer(np.zeros((1, 16385), np.float32), np.zeros(16385, np.float32), np.ones(16385, np.float32))
    # the longest and widest layer, in both loops: LDS raised past 64 KiB
    for rows in ("f32", "f64"):
        T = mc.LOOPS[rows]
        x = np.ones((3, mc.N_MAX), T)
        w = np.zeros((mc.N_MAX, mc.M_MAX), T)
        w[:, 255], w[::2, 7] = 1, -1
        got = dense_layer_no_bias(x, w, "t")
        assert got.shape == (3, 256) and (got[:, 255] == 1).all() and (got[:, 7] == -1).all() and (np.delete(got, [7, 255], axis=1) == 0).all()
    for m, count, blocks in ((17, 64, 1), (17, 65, 2), (256, 130, 3)):
        chain = Chain(mc.program(100, m), compute_dtype=np.float32)
        g = chain.geometry(count)
        assert chain.kernel_name == mc.KERNEL and g["blocks"] == blocks and g["waves_per_block"] == 4 and 4 * g["lds_bytes_per_wave"] == mc.lds_bytes(m, 4), g
        chain.close()


def _recipe(module=M):
    """the docstring's recipe (ml.py:5-32), the two dense layers with weights of their own"""
    return {"layer_1": {"function": "normalisation_layer", "module": module, "args": ["wf_blsub", "db.mean", "db.variance", "layer_1"]},
            "layer_2": {"function": "dense_layer_with_bias", "module": module, "args": ["layer_1", "db.kernel", "db.bias", "'r'", "layer_2"]},
            "classifier": {"function": "dense_layer_with_bias", "module": module, "args": ["layer_2", "db.kernel_2", "db.bias_2", "'s'", "classifier"]},
            "score": {"function": "classification_layer_with_bias", "module": module, "args": ["layer_2", "db.kernel_3", 0.25, "'t'", "score"]}}


def test_the_docstring_recipe_against_the_layers_called_one_by_one():
    from dspeed_amd import processors as P
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    n, count = 100, 70
    x = mc.rows_of("f32", count, n)
    w1, b1, mu, var = mc.layer_of("f32", n, 20)
    w2, b2, _m, _v = mc.layer_of("f32", 20, 3)
    w3 = mc.layer_of("f32", 20, 1)[0][:, 0]
    # (the database holds float64 lists of the float32 values: the recipe casts them back once, exactly)
    db = {"mean": mu.tolist(), "variance": var.tolist(), "kernel": w1.tolist(), "bias": b1.tolist(), "kernel_2": w2.tolist(), "bias_2": b2.tolist(),
          "kernel_3": w3.tolist()}
    tb = {"wf_blsub": WaveformInput(x, 16.0)}
    for outputs, launches in ((["classifier", "score"], 3), (["classifier", "score", "layer_1", "layer_2"], 4)):
        chain, _, out = build_processing_chain({"outputs": outputs, "processors": _recipe(f"{M}.ml" if launches == 4 else M)}, tb, db_dict=db)
        chain.execute()
        assert [k for _w, k in chain.kernels()].count(mc.KERNEL) == launches
        l1 = P.normalisation_layer(x, mu, var)
        l2 = P.dense_layer_with_bias(l1, w1, b1, "r")
        assert _same(out["classifier"], P.dense_layer_with_bias(l2, w2, b2, "s")) and out["classifier"].shape == (count, 3)
        assert _same(out["score"], P.classification_layer_with_bias(l2, w3, np.float32(0.25), "t"))
        if launches == 4:
            assert _same(out["layer_1"], l1) and _same(out["layer_2"], l2)
        assert _same(l2, mc.emulate(x, w1, b1, "r", mu, var))


def test_the_reference_bodys_own_results_where_the_order_cannot_matter():
    """tests/golden/ml_layers.npz: integer-valued rows and weights, every partial sum below 2^24.  'r' (and the unknown character) equals
    the reference body's output in every bit, in both loops; 'l' equals the numba-typed emulation (the fixture's numpy2_l is what CPython
    computes with a float32 0.01); the normalisation equals the body's, IEEE division and square root"""
    import json
    import os

    from dspeed_amd import processors as P

    z = np.load(os.path.join(mc.ROOT, "tests", "golden", f"{mc.BOOK}.npz"))
    assert len(json.loads(str(z["__index__"]))) == 2 * len(mc.FIXTURE_SHAPES)
    for n, m in mc.FIXTURE_SHAPES:
        x64, w64, b64 = mc.fixture_layer(n, m)
        for loop, T in (("f32", np.float32), ("f64", np.float64)):
            case = f"{loop}_n{n}_m{m}"
            x, w, b = x64.astype(T), w64.astype(T), b64.astype(T)
            for act in "r" + mc.UNKNOWN:
                assert _same(P.dense_layer_no_bias(x, w, act), z[f"{case}/dense/{act}"]), (case, act)
                assert _same(P.dense_layer_with_bias(x, w, b, act), z[f"{case}/dense_bias/{act}"]), (case, act)
                assert _same(P.classification_layer_no_bias(x, w[:, 0], act), z[f"{case}/class/{act}"]), (case, act)
                assert _same(P.classification_layer_with_bias(x, w[:, 0], b[0], act), z[f"{case}/class_bias/{act}"]), (case, act)
            assert _same(P.dense_layer_with_bias(x, w, b, "l"), mc.emulate(x, w, b, "l")), case
            if T is np.float64:
                assert _same(P.dense_layer_with_bias(x, w, b, "l"), z[f"{case}/dense_bias/l"]), case
            mu, var = (a.astype(T) for a in mc.fixture_norm(n))
            assert _same(P.normalisation_layer(x, mu, var), z[f"{case}/normalised"]), case
            for act in "st":  # (NumPy's exp and tanh in the fixture, another library's on the device: the bound; 'm' of these sums overflows float32's exp)
                assert mc.within(P.dense_layer_with_bias(x, w, b, act), x, w, b, act)[0], (case, act)
