"""tests/ml_cases.py on the CPU: the emulation of the device's rule (one fma chain per output, tests/ml_fma.cpp) against the reference
body's own results (tests/golden/ml_layers.npz, written by tools/gen_golden_ml.py from integer-valued layers whose sums are exact in any
order), the dot product's bound holding for NumPy's own np.dot, and the measurement behind the activation term of that bound."""
import json
import os

import numpy as np
import pytest

import ml_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", f"{mc.BOOK}.npz"))
    return z, {e["case"]: e for e in json.loads(str(z["__index__"]))}


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


def test_the_fixture_is_the_books():
    z = np.load(os.path.join(ROOT, "tests", "golden", f"{mc.BOOK}.npz"))
    index = json.loads(str(z["__index__"]))
    assert [e["case"] for e in index] == [f"{loop}_n{n}_m{m}" for n, m in mc.FIXTURE_SHAPES for loop in ("f32", "f64")]
    assert all(e["kernel"] == mc.KERNEL for e in index) and os.path.getsize(os.path.join(ROOT, "tests", "golden", f"{mc.BOOK}.npz")) < 1 << 20
    for n, m in mc.FIXTURE_SHAPES:  # every partial sum of the fixture is an integer below 2^24: exact in float32 in any order
        x, w, b = mc.fixture_layer(n, m)
        assert np.abs(x).max() <= 1024 and np.abs(w).max() <= 8 and n <= 1024 and (np.abs(x) @ np.abs(w)).max() + np.abs(b).max() < 2 ** 24


@pytest.mark.parametrize("loop, T", [("f32", np.float32), ("f64", np.float64)])
def test_the_emulation_equals_the_reference_body_where_the_order_cannot_matter(golden, loop, T):
    """'r', 't' and the unknown character under their own names; the others as CPython with NumPy 2 types them (numpy2_*), which the
    emulation reproduces with typing="numpy2" -- the same chain, the same bias, another rounding of the activation.  In the float32 loop
    the numba-typed 'l' differs from the recorded numpy2_l somewhere (0.01 is not a float32)."""
    z, index = golden
    differs = False
    for n, m in mc.FIXTURE_SHAPES:
        case = f"{loop}_n{n}_m{m}"
        x64, w64, b64 = mc.fixture_layer(n, m)
        x, w, b = x64.astype(T), w64.astype(T), b64.astype(T)
        for act in mc.ACTIVATIONS + mc.UNKNOWN:
            name = act if act in "rt" + mc.UNKNOWN or T is np.float64 else f"numpy2_{act}"
            typing = "numpy2" if name.startswith("numpy2") else "numba"
            exact_fn = act in "rl" + mc.UNKNOWN  # (exp, log and tanh are NumPy's in the fixture and in the emulation alike: the same build, the same bits)
            for key, ww, bb in (("dense", w, None), ("dense_bias", w, b), ("class", w[:, 0], None), ("class_bias", w[:, 0], b[0])):
                want = z[f"{case}/{key}/{name}"]
                got = mc.emulate(x, ww, bb, act, typing=typing)
                assert _same(got, want), (case, key, act)
                if loop == "f32" and act == "l" and exact_fn:
                    differs |= not _same(mc.emulate(x, ww, bb, act), want)
        mu, var = (a.astype(T) for a in mc.fixture_norm(n))
        assert _same(mc.normalise(x, mu, var), z[f"{case}/normalised"])
    assert differs == (loop == "f32")


def test_numpys_own_dot_meets_the_dot_products_bound():
    """|np.dot - exact| <= (n + 2) u (sum |x w| + |b|), the bound without its activation term, for BLAS's order of summation; and with the
    reference's activations behind it, the whole bound"""
    worst = 0.0
    for rows in mc.ROWS:
        T = mc.LOOPS[rows]
        for n, m, count in mc.shapes(rows):
            x = mc.rows_of(rows, count, n)
            w, b, _mu, _var = mc.layer_of(rows, n, m)
            pre = (x.astype(T) @ w + b).astype(T)
            val, mag = mc.exact(x, w, b, "r")
            W = mc._wide(T)
            val = (x.astype(T).astype(W) @ w.astype(W)) + b.astype(W)  # (the pre-activation itself)
            ratio = np.asarray(np.abs(pre.astype(W) - val), dtype=np.float64) / ((n + 2) * mc.U[np.dtype(T)] * np.asarray(mag, dtype=np.float64))
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (rows, n, m, float(ratio.max()))
            for act in mc.ACTIVATIONS:
                ok, r = mc.within(mc.activate(pre, act), x, w, b, act)
                assert ok, (rows, n, m, act, r)
    print(f"np.dot: worst |dot - exact| / ((n + 2) u sum|x w|) = {worst:.3f}")


def test_the_measurement_behind_the_activation_term():
    """the figures beside MEASURED_ACT_ULPS: measured here again, printed, and held to the table (not above it; not below half of it, which
    would say the table is stale)"""
    measured = mc.activation_distances()
    print("activation distances in ulps:", {k: {a: round(v, 2) for a, v in d.items()} for k, d in measured.items()})
    for loop, table in mc.MEASURED_ACT_ULPS.items():
        for act in "smt":
            assert table[act] / 2 <= measured[loop][act] <= table[act], (loop, act, measured[loop][act])
        assert measured[loop]["r"] == 0 and measured[loop]["l"] == 0
    assert mc.FACTOR == 2.0 and mc.act_ulps(np.float32, "r") == 2.0 and mc.act_ulps(np.float32, "s") == 2 * mc.MEASURED_ACT_ULPS["f32"]["s"]


def test_the_chain_program_is_an_fma_chain_and_not_a_product_and_add():
    """three terms whose fused sum differs from the twice-rounded one"""
    x = np.array([[1.0, 1 + 2.0 ** -12]], np.float32)
    w = np.array([[-1.0], [1 + 2.0 ** -12]], np.float32)
    fused = mc.chain(x, w)[0, 0]
    assert fused == np.float32(2.0 ** -11 + 2.0 ** -24) and np.float32(x[0, 1] * w[1, 0]) + np.float32(-1.0) == np.float32(2.0 ** -11)
    x64, w64 = x.astype(np.float64) + 2.0 ** -40, w.astype(np.float64)
    assert mc.chain(x64, w64).dtype == np.float64
