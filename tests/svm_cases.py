"""The case book of svm_predict (reference processors/svm.py:13-71), its emulation in float64 NumPy and the derived tolerance of a decision.
A plain helper: tests/test_svm_cases_cpu.py holds the book to its own claims (and to scikit-learn where that is installed),
tests/test_svm_plan_cpu.py and tests/test_gpu_svm.py read it.

A model is a dict of the arrays a fitted ``sklearn.svm.SVC`` holds (``dspeed_amd.processors.svm_model_arrays``): ``kernel`` ("rbf" or
"linear"), ``gamma``, ``support_vectors`` (n_sv, n), ``n_support`` (k,), ``dual_coef`` (k - 1, n_sv: the underscored attribute),
``intercept`` (k (k - 1) / 2: the underscored one) and ``classes`` (k,).  The book's models are synthetic arrays: nothing is trained here.

The rule (libsvm's one-vs-one predict): the support vectors are grouped by class in class order; K_s = exp(-gamma |x - sv_s|^2) or x . sv_s;
for every pair p = (i, j), i < j, in the order (0,1), (0,2) .. (k-2,k-1)
    dec_p = sum_{cls(s) = i} dual_coef[j - 1, s] K_s + sum_{cls(s) = j} dual_coef[i, s] K_s + intercept[p]
dec_p > 0 votes for i, anything else for j; the label is classes[c] of the first class with the most votes.  A row with a NaN gives NaN;
so does, on the device, a row with an infinite sample (scikit-learn raises ValueError there)."""
import numpy as np

EPS = 2.0 ** -52
N_MAX, CLASSES_MAX = 16384, 23
LIMITS = f"rows of up to {N_MAX} samples and models of up to {CLASSES_MAX} classes"
KERNEL = "dsp_svm_kernel"


def pairs(k):
    return [(i, j) for i in range(k) for j in range(i + 1, k)]


def class_of(model):
    """the class of every support vector"""
    return np.repeat(np.arange(len(model["n_support"])), model["n_support"])


def coef_matrix(model, swapped=False):
    """D (n_sv, P): the coefficient of support vector s in pair p, 0 where its class is not in the pair"""
    cls, k = class_of(model), len(model["classes"])
    dual = np.asarray(model["dual_coef"], dtype=np.float64)
    D = np.zeros((len(cls), k * (k - 1) // 2))
    for p, (i, j) in enumerate(pairs(k)):
        ri, rj = (i, j - 1) if swapped else (j - 1, i)
        D[cls == i, p] = dual[ri, cls == i]
        D[cls == j, p] = dual[rj, cls == j]
    return D


def kernel_values(model, rows, gamma=None):
    """K (rows, n_sv) in float64, the distances from direct differences as libsvm forms them"""
    x, sv = np.asarray(rows, dtype=np.float64), np.asarray(model["support_vectors"], dtype=np.float64)
    with np.errstate(all="ignore"):
        if model["kernel"] == "linear":
            return x @ sv.T
        g = float(model["gamma"]) if gamma is None else gamma
        d2 = ((x[:, None, :] - sv[None, :, :]) ** 2).sum(axis=2)
        return np.exp(-g * d2)


def emulate(model, rows, *, public_sign=False, vote_ge=False, last_max=False, order_ji=False, swapped=False, no_gamma=False):
    """(labels, decisions) in float64; the keywords are the rule's wrong neighbours, one at a time (tests/test_svm_cases_cpu.py)"""
    rows = np.atleast_2d(np.asarray(rows))
    k = len(model["classes"])
    order = pairs(k)
    D, icpt = coef_matrix(model, swapped), np.asarray(model["intercept"], dtype=np.float64)
    if public_sign and k == 2:
        D, icpt = -D, -icpt
    if order_ji:  # the pairs' columns enumerated by (j, i) against intercepts that stay where they are
        by_ji = sorted(range(len(order)), key=lambda p: (order[p][1], order[p][0]))
        D = D[:, by_ji]
        order = [order[p] for p in by_ji]
    with np.errstate(all="ignore"):
        dec = kernel_values(model, rows, 1.0 if no_gamma else None) @ D + icpt
    nonfinite = ~np.isfinite(rows.astype(np.float64)).all(axis=1)
    dec[nonfinite] = np.nan
    votes = np.zeros((len(rows), k), dtype=np.int64)
    for p, (i, j) in enumerate(order):
        for_i = dec[:, p] >= 0 if vote_ge else dec[:, p] > 0
        votes[:, i] += for_i
        votes[:, j] += ~for_i
    c = k - 1 - np.argmax(votes[:, ::-1], axis=1) if last_max else np.argmax(votes, axis=1)
    labels = np.asarray(model["classes"], dtype=np.float64)[c]
    labels[np.isnan(dec).any(axis=1)] = np.nan
    return labels, dec


def bound(model, rows):
    """the tolerance of a decision, per row and pair: the rounding of the expansion |x|^2 + |sv|^2 - 2 x.sv, of an exponential taken as 1 ulp
    and of a sum of n_sv terms in any order; the factor 4 is for the device's exp and for contraction"""
    x, sv = np.atleast_2d(np.asarray(rows, dtype=np.float64)), np.asarray(model["support_vectors"], dtype=np.float64)
    n_sv, n = sv.shape
    absD, icpt = np.abs(coef_matrix(model)).sum(axis=0), np.abs(np.asarray(model["intercept"], dtype=np.float64))
    with np.errstate(all="ignore"):
        x2, sv2 = (x ** 2).sum(axis=1), (sv ** 2).sum(axis=1).max()
        if model["kernel"] == "linear":
            per_term = (n + 4) * np.sqrt(x2) * np.sqrt(sv2) + n_sv + 8
        else:
            per_term = 2 * float(model["gamma"]) * (n + 4) * (x2 + sv2) + n_sv + 8
        return 4 * EPS * (absD[None, :] * per_term[:, None] + icpt[None, :])


# ---------------------------------------------------------------------------------------------------------------- the book
def synthetic(seed, n, n_sv, k, kernel, classes=None):
    """a model of random arrays: uneven n_support with classes of one support vector, decisions of order 1"""
    rng = np.random.default_rng(seed)
    n_support = np.ones(k, dtype=np.int32)
    extra = n_sv - k
    assert extra >= 0
    if extra:
        share = rng.multinomial(extra, rng.dirichlet(np.full(k, 0.5)))
        share[0], share[-1] = 0, share[-1] + share[0]  # (class 0 keeps its single support vector wherever there is a choice)
        n_support += share.astype(np.int32)
    P = k * (k - 1) // 2
    return {"kernel": kernel, "gamma": 2.0 / n, "support_vectors": rng.standard_normal((n_sv, n)),
            "n_support": n_support, "dual_coef": rng.standard_normal((k - 1, n_sv)) * (1.0 if kernel == "rbf" else 1.0 / np.sqrt(n)),
            "intercept": rng.standard_normal(P) * 0.5,
            "classes": np.arange(k, dtype=np.float64) if classes is None else np.asarray(classes, dtype=np.float64)}


def _rows(seed, count, n, dtype, near=None):
    """random rows; with ``near``, each beside one of those support vectors, so that its K stands out and the labels vary"""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((count, n))
    if near is None:
        return noise.astype(dtype)
    return (near[rng.integers(0, len(near), count)] + 0.3 * noise).astype(dtype)


#: (name, n, n_sv, k, kernel, rows, row type, class values): every n, n_sv, k and row count of the issue's lists, both kernels and both types
SHAPES = (
    ("n1", 1, 2, 2, "rbf", 1, np.float32, None),
    ("n3", 3, 15, 3, "linear", 15, np.float32, (1, 3, 5)),
    ("n4", 4, 16, 4, "rbf", 16, np.float64, (-2, 0, 1.5, 7)),
    ("n5", 5, 17, 16, "linear", 17, np.float32, None),
    ("n63", 63, 64, 16, "rbf", 63, np.float32, tuple(range(-5, 27, 2))),
    ("n64", 64, 65, 4, "linear", 64, np.float64, None),
    ("n65", 65, 300, 16, "rbf", 65, np.float32, None),
    ("n257", 257, 300, 3, "rbf", 129, np.float32, (-1, 4, 9)),
    ("n257_linear", 257, 65, 2, "linear", 129, np.float64, (3, -3)),
    ("n64_two", 64, 300, 2, "rbf", 17, np.float64, None),
)


def named_model():
    """n = 5, 17 support vectors, 3 classes, rbf; intercepts (+5, -5, +5): where every K underflows each class gets one vote and the first wins"""
    m = synthetic(101, 5, 17, 3, "rbf", classes=(1, 3, 5))
    m["intercept"] = np.array([5.0, -5.0, 5.0])
    return m


def named_rows(model):
    """{name: row index} and the float32 rows: NaNs first and last beside clean rows on one tile, infinities, zeros, a support vector, a far row"""
    n = model["support_vectors"].shape[1]
    rows = _rows(102, 20, n, np.float32)
    names = {"nan_first": 0, "clean_beside": 1, "nan_last": 2, "plus_inf": 3, "minus_inf": 4, "zeros": 5, "support_vector": 6, "far_tie": 7, "nan_all": 19}
    rows[0, 0] = np.nan
    rows[2, -1] = np.nan
    rows[3, 1] = np.inf
    rows[4, 2] = -np.inf
    rows[5] = 0.0
    rows[6] = model["support_vectors"][4].astype(np.float32)
    rows[7] = 100.0
    rows[19] = np.nan
    return names, rows


def exact_zero_case():
    """linear, small integers: both sides compute dec exactly; row 1's is exactly 0 and the vote goes to j, the second class"""
    model = {"kernel": "linear", "gamma": 0.25, "support_vectors": np.array([[1.0, 2.0, 0.0], [0.0, -1.0, 3.0], [2.0, 0.0, 1.0]]),
             "n_support": np.array([1, 2], dtype=np.int32), "dual_coef": np.array([[2.0, -1.0, -3.0]]), "intercept": np.array([4.0]),
             "classes": np.array([10.0, 20.0])}
    # K = (x.sv0, x.sv1, x.sv2); dec = 2 K0 - K1 - 3 K2 + 4
    rows = np.array([[1.0, 1.0, 1.0],     # 6 - 2 - 9 + 4 = -1: class 20
                     [1.0, 0.0, 0.0],     # 2 - 0 - 6 + 4 = 0 exactly: class 20
                     [0.0, 3.0, 0.0]],    # 12 + 3 - 0 + 4 = 19: class 10
                    dtype=np.float32)
    return model, rows, 1


def cases():
    """[(name, model, rows)]: the shapes, the named rows on their model, the exact zero"""
    out = []
    for k, (name, n, n_sv, n_cls, kernel, count, dtype, classes) in enumerate(SHAPES):
        model = synthetic(10 + k, n, n_sv, n_cls, kernel, classes)
        out.append((name, model, _rows(50 + k, count, n, dtype, model["support_vectors"] if kernel == "rbf" else None)))
    m = named_model()
    out.append(("named", m, named_rows(m)[1]))
    zm, zr, _ = exact_zero_case()
    out.append(("exact_zero", zm, zr))
    return out


def host_arrays(model):
    """what the device takes, float64 and contiguous: support vectors, their squared norms, D, intercepts, classes"""
    sv = np.ascontiguousarray(model["support_vectors"], dtype=np.float64)
    return (sv, np.ascontiguousarray((sv * sv).sum(axis=1)), np.ascontiguousarray(coef_matrix(model)),
            np.ascontiguousarray(model["intercept"], dtype=np.float64), np.ascontiguousarray(model["classes"], dtype=np.float64))


def program(n, n_sv, k, rows=np.float32, loop=np.float32, kind=0, gamma=0.5, decisions=False, row_stride=None):
    """LOAD, SVM_PREDICT, STORE_SCALAR as the entry point and the recipe compiler write them; the model's bindings are float64 in both loops"""
    from dspeed_amd import _lib
    from dspeed_amd.chain import Program, Scalar

    P = k * (k - 1) // 2
    p = Program()
    s = p.add_slot(n)
    p.add_op(_lib.OP_LOAD, dst=s, io=p.add_io("in", _lib.IO_WF_IN, rows, n, 0, row_stride))
    ios = [p.add_io(name, _lib.IO_TAPS, np.float64, length, 0, 0)
           for name, length in (("support_vectors", n_sv * n), ("sv_norms", n_sv), ("coefficients", n_sv * P), ("intercepts", P), ("classes", k))]
    dec = p.add_io("decisions", _lib.IO_WF_OUT, np.float64, P, 0, P) if decisions else -1
    r = p.add_sregs(1)
    p.add_op(_lib.OP_SVM_PREDICT, dst=r, src=s, io=ios[0], ip=tuple(ios[1:]), sp=(Scalar.const(gamma), Scalar.const(kind), Scalar.const(dec)))
    p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("label", _lib.IO_SCALAR_OUT, loop), ip=(r,))
    return p
