"""The case book of svm_predict (tests/svm_cases.py) held to its own claims without a device: every finite row is decided, so labels compare
without exemptions; the emulation is scikit-learn's predict and decision_function where scikit-learn is installed, and the recorded
fixture's everywhere; each wrong neighbour of the rule fails on the book."""
import os

import numpy as np
import pytest

import svm_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "svm.npz")


def test_every_finite_row_of_the_book_is_decided():
    """|dec_p| >= 1000 x its bound in every finite row but the one exact zero: no row is left out of a label comparison"""
    left_out, rows_seen = 0, 0
    _, _, zero_row = sc.exact_zero_case()
    for name, model, rows in sc.cases():
        labels, dec = sc.emulate(model, rows)
        tol = sc.bound(model, rows)
        finite = np.isfinite(rows.astype(np.float64)).all(axis=1)
        assert np.array_equal(np.isnan(labels), ~finite) and np.array_equal(np.isnan(dec).all(axis=1), ~finite), name
        for r in np.flatnonzero(finite):
            rows_seen += 1
            if name == "exact_zero" and r == zero_row:
                assert dec[r, 0] == 0.0 and labels[r] == model["classes"][1]  # the vote goes to j
                continue
            left_out += not (np.abs(dec[r]) >= 1000 * tol[r]).all()
    assert rows_seen > 400 and left_out / rows_seen == 0.0


def test_the_book_meets_every_edge_the_issue_lists():
    shapes = sc.cases()
    ns = {m["support_vectors"].shape[1] for _, m, _ in shapes}
    assert {1, 3, 4, 5, 63, 64, 65, 257} <= ns
    assert {2, 15, 16, 17, 64, 65, 300} <= {m["support_vectors"].shape[0] for _, m, _ in shapes}
    assert {2, 3, 4, 16} <= {len(m["classes"]) for _, m, _ in shapes}
    assert {1, 15, 16, 17, 63, 64, 65, 129} <= {len(r) for _, _, r in shapes}
    assert {m["kernel"] for _, m, _ in shapes} == {"rbf", "linear"} and {r.dtype for _, _, r in shapes} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any((m["n_support"] == 1).any() and (m["n_support"] > 1).any() for _, m, _ in shapes)
    assert any(not np.array_equal(m["classes"], np.arange(len(m["classes"]))) and (m["classes"] < 0).any() for _, m, _ in shapes)
    model = sc.named_model()
    names, rows = sc.named_rows(model)
    labels, dec = sc.emulate(model, rows)
    assert np.isnan(rows[names["nan_first"], 0]) and np.isnan(rows[names["nan_last"], -1]) and np.isfinite(rows[names["clean_beside"]]).all()
    assert np.array_equal(dec[names["far_tie"]], model["intercept"]) and labels[names["far_tie"]] == model["classes"][0]  # every K underflows: a vote each
    assert (rows[names["zeros"]] == 0).all() and np.array_equal(rows[names["support_vector"]], model["support_vectors"][4].astype(np.float32))


@pytest.mark.parametrize("neighbour", ["public_sign", "vote_ge", "last_max", "order_ji", "swapped", "no_gamma"])
def test_each_wrong_neighbour_of_the_rule_fails_on_the_book(neighbour):
    wrong = []
    for name, model, rows in sc.cases():
        labels, _ = sc.emulate(model, rows)
        other, _ = sc.emulate(model, rows, **{neighbour: True})
        if not np.array_equal(labels, other, equal_nan=True):
            wrong.append(name)
    assert wrong, f"{neighbour}: no label of the book changes"


def _fixture_models():
    with np.load(GOLDEN) as f:
        for name in sorted({key.split("/")[0] for key in f.files}):
            model = {field: f[f"{name}/{field}"] for field in ("support_vectors", "n_support", "dual_coef", "intercept", "classes")}
            model["kernel"], model["gamma"] = str(f[f"{name}/kernel"]), float(f[f"{name}/gamma"])
            yield name, model, f[f"{name}/rows"], f[f"{name}/labels"], f[f"{name}/decisions"]


def test_the_emulation_is_the_recorded_scikit_learn():
    seen = set()
    for name, model, rows, labels, dec in _fixture_models():
        got_l, got_d = sc.emulate(model, rows)
        scale = np.abs(sc.coef_matrix(model)).sum(axis=0) + np.abs(model["intercept"])
        assert np.array_equal(got_l, labels), name
        assert (np.abs(got_d - dec) <= 1e-12 * scale).all(), (name, float(np.abs(got_d - dec).max()))
        seen.add((len(model["classes"]), model["kernel"]))
    assert seen == {(k, kern) for k in (2, 3, 5) for kern in ("rbf", "linear")}


def test_the_emulation_is_scikit_learn_on_trained_models():
    pytest.importorskip("sklearn")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_golden_svm as gen
    finally:
        sys.path.pop(0)
    from dspeed_amd.processors import svm_model_arrays

    for i, (name, k, n, kernel, gamma, values) in enumerate(gen.MODELS):
        svc, rows = gen.trained(2000 + i, k, n, kernel, gamma, values)
        model = svm_model_arrays(svc)
        labels, dec = sc.emulate(model, rows)
        want = np.asarray(svc.decision_function(rows.astype(np.float64))).reshape(len(rows), -1) * (-1 if k == 2 else 1)
        scale = np.abs(sc.coef_matrix(model)).sum(axis=0) + np.abs(model["intercept"])
        assert (np.abs(dec - want) <= 1e-12 * scale).all(), name
        decided = (np.abs(dec) >= 1000 * sc.bound(model, rows)).all(axis=1)
        assert decided.sum() > 40 and np.array_equal(labels[decided], svc.predict(rows.astype(np.float64))[decided].astype(np.float64)), name
