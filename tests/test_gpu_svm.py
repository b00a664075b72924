"""svm_predict on the device (dsp_svm.hip): the book of tests/svm_cases.py through the C entry -- both loops, padded row strides (the scalar
loader) and whole vectors, every n, n_sv, class count and row count at which the kernel takes another path, with a sentinel around the
labels and behind every decisions row --, the recorded scikit-learn models of tests/golden/svm.npz, the gufunc and the recipe stage.

Labels equal the emulation's in every row (the book's rows are decided: tests/test_svm_cases_cpu.py), with the same NaN pattern and type;
decisions stay within ``svm_cases.bound``.  Nothing here imports scikit-learn."""
import os

import numpy as np
import pytest

import svm_cases as sc

pytestmark = pytest.mark.gpu

M = "dspeed.processors"
SENTINEL = -7.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm.npz")


def _predict(model, rows, loop, pad=0, with_dec=True):
    """(labels, decisions or None, everything else the call left in the two buffers) of dsp_svm_rows on rows n + pad apart"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.gufunc import run

    count, n = rows.shape
    k = len(model["classes"])
    P = k * (k - 1) // 2
    block = np.full((count, n + pad), 77, dtype=rows.dtype)
    block[:, :n] = rows
    host = sc.host_arrays(model)
    dev = [DeviceArray.from_numpy(a) for a in host]
    d_rows = DeviceArray.from_numpy(block)
    l_off, d_off, d_stride = 1 + 2 * (count % 2), 1, P + 3
    labels = DeviceArray.from_numpy(np.full(l_off + count + 5, SENTINEL, dtype=loop))
    decs = DeviceArray.from_numpy(np.full(d_off + count * d_stride + 4, SENTINEL, dtype=np.float64))
    run(_lib.lib().dsp_svm_rows, "svm_predict", d_rows.ptr, _lib.F32 if rows.dtype == np.float32 else _lib.F64, count, n, n + pad,
        _lib.F32 if loop is np.float32 else _lib.F64, *(d.ptr for d in dev), host[0].shape[0], k, sc_kind(model), float(model["gamma"]),
        labels.ptr + l_off * np.dtype(loop).itemsize, decs.ptr + d_off * 8 if with_dec else None, d_stride)
    got_l, got_d = labels.to_numpy(), decs.to_numpy()
    body = got_d[d_off:d_off + count * d_stride].reshape(count, d_stride)
    rest = np.concatenate([got_l[:l_off], got_l[l_off + count:], got_d[:d_off], got_d[d_off + count * d_stride:], body[:, P:].reshape(-1)])
    if not with_dec:
        rest = np.concatenate([rest, body[:, :P].reshape(-1)])
    return got_l[l_off:l_off + count], (body[:, :P] if with_dec else None), rest


def sc_kind(model):
    return ("rbf", "linear").index(model["kernel"])


def _check(name, model, rows, loop, pad, worst):
    want_l, want_d = sc.emulate(model, rows)
    tol = sc.bound(model, rows)
    labels, dec, rest = _predict(model, rows, loop, pad)
    assert (rest == SENTINEL).all(), f"{name}: something but the labels and the decisions was written"
    assert labels.dtype == np.dtype(loop)
    assert np.array_equal(labels, want_l.astype(loop), equal_nan=True), (name, labels[:8], want_l[:8])
    assert np.array_equal(np.isnan(dec), np.isnan(want_d)), name
    fin = np.isfinite(want_d)
    err = np.abs(dec - want_d)[fin]
    print(f"{name} ({np.dtype(loop).name} loop, pad {pad}): worst decision error / bound {float((err / tol[fin]).max()) if err.size else 0.0:.3f}")
    assert (err <= tol[fin]).all(), (name, float((err / tol[fin]).max()))
    if err.size:
        worst.append(float((err / tol[fin]).max()))
    again, none, rest = _predict(model, rows, loop, pad, with_dec=False)
    assert none is None and (rest == SENTINEL).all() and np.array_equal(again, labels, equal_nan=True), f"{name}: the labels without the decisions"


@pytest.mark.parametrize("pad", [0, 3])
def test_the_whole_book_through_the_c_entry_with_sentinels(pad):
    worst = []
    for name, model, rows in sc.cases():
        loop = np.float32 if rows.dtype == np.float32 else np.float64
        _check(name, model, rows, loop, pad, worst)
        if rows.dtype == np.float32 and name in ("n3", "n65", "named"):  # float32 rows in the float64 loop: the label is a float64
            _check(name + "/f64 loop", model, rows, np.float64, pad, worst)
    print(f"worst decision error over the book, in bounds: {max(worst):.3f}")


def test_the_named_rows_by_name():
    model = sc.named_model()
    names, rows = sc.named_rows(model)
    labels, dec, _ = _predict(model, rows, np.float32)
    for nan_row in ("nan_first", "nan_last", "plus_inf", "minus_inf", "nan_all"):
        assert np.isnan(labels[names[nan_row]]) and np.isnan(dec[names[nan_row]]).all(), nan_row
    assert np.isfinite(labels[names["clean_beside"]]) and np.isfinite(dec[names["clean_beside"]]).all()
    assert np.array_equal(dec[names["far_tie"]], model["intercept"]) and labels[names["far_tie"]] == model["classes"][0]  # a vote each: the first class
    zm, zr, at = sc.exact_zero_case()
    labels, dec, _ = _predict(zm, zr, np.float32)
    assert dec[at, 0] == 0.0 and labels[at] == zm["classes"][1] and np.array_equal(dec[:, 0], [-1.0, 0.0, 19.0])


def test_the_recorded_scikit_learn_models():
    with np.load(GOLDEN) as f:
        names = sorted({key.split("/")[0] for key in f.files})
        for name in names:
            model = {field: f[f"{name}/{field}"] for field in ("gamma", "support_vectors", "n_support", "dual_coef", "intercept", "classes")}
            model["kernel"], model["gamma"] = str(f[f"{name}/kernel"]), float(model["gamma"])
            rows, want_l, want_d = f[f"{name}/rows"], f[f"{name}/labels"], f[f"{name}/decisions"]
            labels, dec, _ = _predict(model, rows, np.float32 if rows.dtype == np.float32 else np.float64)
            assert np.array_equal(labels.astype(np.float64), want_l.astype(np.float64)), name
            ratio = float((np.abs(dec - want_d) / sc.bound(model, rows)).max())
            print(f"{name}: worst decision error against scikit-learn's recorded decisions / bound {ratio:.3f}")
            assert (np.abs(dec - want_d) <= sc.bound(model, rows)).all(), (name, ratio)


def test_the_gufunc_on_device_and_host_arrays():
    from dspeed_amd import processors
    from dspeed_amd.device import DeviceArray

    name, model, rows = next(c for c in sc.cases() if c[0] == "n65")
    want, _ = sc.emulate(model, rows)
    g = processors.svm_predict(dict(model))
    assert (g.signature, g.types) == ("(n)->()", ["f->f", "d->d"])
    got = g(rows)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    held = [d.ptr for d in g.device_arrays]
    out = DeviceArray((len(rows),), np.float32)
    assert g(DeviceArray.from_numpy(rows), out) is out and np.array_equal(out.to_numpy(), got)
    assert [d.ptr for d in g.device_arrays] == held and len(held) == 5  # the same processor again: no new upload of the model
    one = g(rows[3])
    assert np.ndim(one) == 0 and one == got[3]
    assert np.array_equal(g(rows.astype(np.float64)), want) and g(rows.astype(np.float64)).dtype == np.float64
    null = processors.svm_predict(0)
    assert np.isnan(null(rows)).all() and null(rows).shape == (len(rows),)
    with pytest.raises(ValueError, match="the rows hold 64 samples, the model's support vectors 65"):
        g(rows[:, :64])


def test_chains_of_different_lds_sizes_side_by_side():
    """rows of 256 samples (146 KiB of LDS), then of 128 (82 KiB), then the first chain again: the kernels' dynamic-LDS limit is raised once to
    the largest any chain needs, so the later, smaller chain does not undercut the launch of the earlier one"""
    from dspeed_amd import processors

    wide, narrow = sc.synthetic(5, 256, 70, 3, "rbf"), sc.synthetic(6, 128, 70, 3, "rbf")
    rows_w, rows_n = sc._rows(7, 65, 256, np.float32, wide["support_vectors"]), sc._rows(8, 65, 128, np.float32, narrow["support_vectors"])
    g_w, g_n = processors.svm_predict(wide), processors.svm_predict(narrow)
    first = g_w(rows_w)
    assert np.array_equal(g_n(rows_n), sc.emulate(narrow, rows_n)[0].astype(np.float32))
    assert np.array_equal(g_w(rows_w), first) and np.array_equal(first, sc.emulate(wide, rows_w)[0].astype(np.float32))


RECIPE = {
    "outputs": ["label", "is_clean"],
    "processors": {
        "dwt": {"function": "discrete_wavelet_transform", "module": M, "args": ["waveform", 2, "'h'", "'a'", "dwt(64)"]},
        "dwt_norm": {"function": "normalisation_layer", "module": M, "args": ["dwt", "db.means", "db.variances", "dwt_norm"]},
        "label": {"function": "svm_predict", "module": M, "args": ["dwt_norm", "label"], "init_args": ["db.svm_file"]},
        "is_clean": "where(label == 3, 1, 0)",
    },
}


def _row_margin(model, rows, ulps=4):
    """What a decision may move when every sample of a float32 row moves by up to ``ulps`` units in its last place (the device's transform
    and normalisation against the oracle's): |dx| <= delta = ulps 2^-23 |x|, the squared distance to a support vector at distance d moves by
    at most 2 d delta + delta^2, K = exp(-gamma d^2) <= 1 has a slope of at most gamma in d^2, and a decision sums |D[s, p]| of them."""
    x, sv = rows.astype(np.float64), model["support_vectors"]
    delta = ulps * 2.0 ** -23 * np.sqrt((x ** 2).sum(axis=1))
    d = np.sqrt(((x[:, None, :] - sv[None, :, :]) ** 2).sum(axis=2))
    return (model["gamma"] * (2 * d * delta[:, None] + delta[:, None] ** 2)) @ np.abs(sc.coef_matrix(model))


def test_a_recipe_through_both_builders(tmp_path):
    """discrete_wavelet_transform -> normalisation_layer -> svm_predict -> an expression on the label, against the emulation applied to the
    oracle's intermediate rows: its Haar transform, normalised in float32 NumPy.  The model is made beside those rows and every decision is
    asserted to clear 1000 bounds plus what 4 float32 units in the last place of every sample can move it (``_row_margin``), so the labels
    do not hang on how the device rounds the rows."""
    import oracle
    from dspeed_amd.build_dsp import build_dsp
    from dspeed_amd.processing_chain import build_processing_chain

    rng = np.random.default_rng(7)
    wf = rng.standard_normal((129, 256)).cumsum(axis=1).astype(np.float32)
    path = str(tmp_path / "model.npz")
    means, variances = rng.standard_normal(64).astype(np.float32), (rng.uniform(0.5, 2.0, 64) * 50).astype(np.float32)
    db = {"means": means.tolist(), "variances": variances.tolist(), "svm_file": f"'{path}'"}
    dwt, rc = oracle.dwt_haar(wf, 2, "a", 64)
    assert rc == 0 and dwt.dtype == np.float32
    norm = (dwt - means) / np.sqrt(variances)
    assert norm.shape == (129, 64) and norm.dtype == np.float32
    model = sc.synthetic(77, 64, 40, 3, "rbf", classes=(1, 3, 5))
    model["support_vectors"] = norm[:120:3].astype(np.float64) + 0.05 * rng.standard_normal((40, 64))  # (beside the rows themselves: the labels vary)
    model["gamma"] = 2.0 / float(np.mean((norm[:-1] - norm[1:]) ** 2) * 64)
    np.savez(path, **model)
    want, dec = sc.emulate(model, norm)
    assert (np.abs(dec) >= 1000 * sc.bound(model, norm) + _row_margin(model, norm)).all() and len(np.unique(want)) > 1  # (decided rows, more than one class)
    chain, _, tb = build_processing_chain(RECIPE, {"waveform": wf}, db_dict=db)
    assert [st["what"] for st in chain._stages][-1] == "svm_predict label on rows"
    chain.execute()
    assert np.array_equal(np.asarray(tb["label"]), want.astype(np.float32))
    assert np.array_equal(np.asarray(tb["is_clean"]), (want == 3).astype(np.asarray(tb["is_clean"]).dtype))
    out = build_dsp({"waveform": wf}, dsp_config=RECIPE, database=db)
    assert np.array_equal(out["label"], want.astype(np.float32)) and np.array_equal(out["is_clean"], np.asarray(tb["is_clean"]))
    null = {"outputs": ["label"], "processors": {"label": {"function": "svm_predict", "module": M, "args": ["waveform", "label"], "init_args": [0]}}}
    chain, _, tb = build_processing_chain(null, {"waveform": wf}, db_dict=db)
    chain.execute()
    assert np.isnan(np.asarray(tb["label"])).all() and np.asarray(tb["label"]).shape == (129,)
