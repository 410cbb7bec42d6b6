"""Shared helpers of the device SVC fit tests (tests/test_svc_fit_cpu.py, tests/test_svc_fit_gpu.py): the cases, scikit-learn's own
``SVC(kernel='precomputed')`` fit of each run live on the same symmetric matrix, and the equality both files hold the fit to."""
import functools
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
sys.path.pop(0)

SEED = G.SEED
BASE = {"probability": True, "class_weight": "balanced", "random_state": SEED}
# kernel key, C: RBF gamma = 1 C = 100 reaches probA_ = -18.77, the steep end of libsvm's sigmoid fit
REAL_KERNELS = [(("rbf", 0.01), 10.0), (("linear", None), 0.1), (("rbf", 1.0), 100.0)]
# what differs by construction between a fit on the rows and libsvm's fit on their kernel matrix: the kernel's name and gamma, the
# support vectors (rows against an empty array) and the three attributes that describe the input's shape -- checked in `on_rows`
ROW_KEYS = ("kernel", "gamma", "support_vectors_", "_gamma", "shape_fit_", "n_features_in_")


def svc(key, C, **kw):
    from sklearn.svm import SVC
    params = dict(BASE, **kw)
    if key == "precomputed":
        return SVC(kernel="precomputed", C=C, **params)
    return SVC(kernel=key[0], C=C, **params) if key[1] is None else SVC(kernel=key[0], gamma=key[1], C=C, **params)


def symmetric(K):
    return np.triu(K) + np.triu(K, 1).T


def five_class():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 5, 200) * 3 + 2                  # labels 2, 5, 8, 11, 14: not class indices
    centers = rng.standard_normal((15, 64))
    X = (centers[y] + 1.5 * rng.standard_normal((200, 64))).astype(np.float32)
    return X, y


def tiny(sizes):
    """40 x 16 rows with the given class sizes: a class of one row (libsvm's +1 / -1 branch: a fold without that class), pairs of
    fewer than five rows (empty folds), classes that miss from single folds"""
    rng = np.random.default_rng(sum(s * 41 ** i for i, s in enumerate(sizes)))
    y = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    y = y[rng.permutation(len(y))]
    X = (rng.standard_normal((len(sizes), 16))[y] + rng.standard_normal((len(y), 16))).astype(np.float32)
    return X, y


TINY_SIZES = [(1, 39), (2, 38), (1, 2, 37), (4, 36)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (X, y, kernel key, C, extra SVC parameters)"""
    X, y = G.real_xy()
    two = y != 0                                         # the 469-row pair: a two-class model (scikit-learn's sign flip)
    out = {}
    for key, C in REAL_KERNELS:
        out["xy-%s-%s-C%s" % (key[0], key[1], C)] = (X, y, key, C, {})
    out["xy-two-class"] = (X[two], y[two], ("rbf", 0.01), 10.0, {})
    X5, y5 = five_class()
    out["five-class"] = (X5, y5, ("rbf", 0.02), 1.0, {})
    for sizes in TINY_SIZES:
        Xt, yt = tiny(sizes)
        out["tiny-%s" % "-".join(map(str, sizes))] = (Xt, yt, ("linear", None), 1.0, {})
    out["no-probability"] = (X, y, ("rbf", 0.01), 10.0, {"probability": False})
    out["max-iter-5"] = (X, y, ("linear", None), 0.1, {"max_iter": 5})
    return out


CASE_NAMES = ["xy-rbf-0.01-C10.0", "xy-linear-None-C0.1", "xy-rbf-1.0-C100.0", "xy-two-class", "five-class"] + \
             ["tiny-%s" % "-".join(map(str, s)) for s in TINY_SIZES] + ["no-probability", "max-iter-5"]


def sklearn_fit(K, y, C, extra):
    """(estimator, warnings) of SVC(kernel='precomputed', ...same parameters...).fit(K, y), run live"""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = svc("precomputed", C, **extra).fit(K, y)
    return m, [x for x in w]


def same_value(a, b, name):
    if isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (name, getattr(a, "dtype", type(a)), b.dtype,
                                                                                         getattr(a, "shape", None), b.shape)
        assert np.array_equal(a, b), (name, a, b)
    else:
        assert type(a) is type(b) and a == b, (name, a, b)


def same_fit(ours, ref, skip=()):
    """the issue's "equal": vars() of the two estimators have the same keys, every array the same dtype, shape and elements, every
    scalar ==; ``skip`` names the keys left to the caller"""
    va, vb = vars(ours), vars(ref)
    assert set(va) == set(vb), sorted(set(va) ^ set(vb))
    for k, v in vb.items():
        if k not in skip:
            same_value(va[k], v, k)


def on_rows(ours, X, key):
    """the attributes of ROW_KEYS: those of a fit on the rows X with this kernel"""
    assert ours.kernel == key[0] and (key[1] is None or ours.gamma == key[1])
    assert ours.shape_fit_ == X.shape and ours.n_features_in_ == X.shape[1]
    assert np.array_equal(ours.support_vectors_, X.astype(np.float64)[ours.support_]) and ours.support_vectors_.dtype == np.float64
    if key[0] == "rbf":
        assert ours._gamma == key[1]
    else:
        var = X.astype(np.float64).var()
        assert ours._gamma == (1.0 / (X.shape[1] * var) if var != 0 else 1.0)              # gamma='scale' as SVC.fit computes it


def check_case(fit_svc, name, case, K):
    """fit_svc on the case's rows against scikit-learn on the matrix K of those rows"""
    X, y, key, C, extra = case
    ref, ref_w = sklearn_fit(K, y, C, extra)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        est = svc(key, C, **extra)
        ours = fit_svc(est, X, y)
    assert ours is est
    same_fit(ours, ref, skip=ROW_KEYS)
    on_rows(ours, X, key)
    assert [str(x.message) for x in w] == [str(x.message) for x in ref_w] and [x.category for x in w] == [x.category for x in ref_w]
    return ours, ref, w
