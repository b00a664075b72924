"""Writes tests/golden/svm.npz: a few small trained ``sklearn.svm.SVC`` models as the arrays of ``svm_model_arrays``, query rows, and what
scikit-learn itself says of them -- ``predict`` and ``decision_function`` in its one-vs-one form (negated for two classes, where the public
sign is the opposite of libsvm's).  From scikit-learn alone: nothing of this project computes anything here.

    python tools/gen_golden_svm.py

Rows whose smallest |decision| lies below 1e-6 are left out, so that a label never hangs on a rounding."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#: (name, classes, samples a row, kernel, gamma, class values)
MODELS = (("two_rbf_scale", 2, 6, "rbf", "scale", (0, 1)), ("three_rbf", 3, 17, "rbf", 0.05, (1, 3, 5)), ("five_rbf_scale", 5, 33, "rbf", "scale", (-2, 0, 1, 4, 9)),
          ("two_linear", 2, 17, "linear", "scale", (3, 7)), ("three_linear", 3, 6, "linear", "scale", (0, 1, 2)), ("five_linear", 5, 33, "linear", 0.1, (0, 1, 2, 3, 4)))


def trained(seed, k, n, kernel, gamma, values):
    from sklearn.svm import SVC

    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, n)) * 1.5
    y = rng.integers(0, k, 40 * k)
    x = centres[y] + rng.standard_normal((len(y), n))
    svc = SVC(kernel=kernel, gamma=gamma, C=1.0, decision_function_shape="ovo").fit(x, np.asarray(values)[y])
    rows = (centres[rng.integers(0, k, 48)] + 1.2 * rng.standard_normal((48, n))).astype(np.float32)
    return svc, rows


def main():
    from dspeed_amd.processors import svm_model_arrays

    out = {}
    for i, (name, k, n, kernel, gamma, values) in enumerate(MODELS):
        svc, rows = trained(1000 + i, k, n, kernel, gamma, values)
        dec = np.asarray(svc.decision_function(rows.astype(np.float64)), dtype=np.float64).reshape(len(rows), -1)
        dec = -dec if k == 2 else dec
        keep = np.abs(dec).min(axis=1) >= 1e-6
        rows, dec = rows[keep], dec[keep]
        for field, value in svm_model_arrays(svc).items():
            out[f"{name}/{field}"] = np.asarray(value)
        out[f"{name}/rows"], out[f"{name}/decisions"] = rows, dec
        out[f"{name}/labels"] = np.asarray(svc.predict(rows.astype(np.float64)), dtype=np.float64)
        print(name, "support vectors", svc.support_vectors_.shape, "rows kept", len(rows))
    path = os.path.join(ROOT, "tests", "golden", "svm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
