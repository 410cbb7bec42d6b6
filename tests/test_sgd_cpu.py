"""The device SGD fit without a GPU: the NumPy twin of csrc/sgd.hip (tests/sgd_common.py) in scikit-learn's summation order against
SGDClassifier run live, the shuffle helper of the library against scikit-learn's, GridSearchSGD / fit_sgd / partial_fit_sgd with the
device hook (``train._sgd``) replaced by the twin, the conditions that make the fixtures valid, and the argument checks."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_common as S  # noqa: E402
sys.path.pop(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


@pytest.mark.parametrize("data,case", S.PAIRS)
def test_twin_is_sklearn(data, case):
    """n_iter_ per class equal, coef_ / intercept_ within 1e-14 max|coef_| (the prototype: <= 3e-16, exactly 0 on several cases);
    and the conditions that make the case a valid fixture: no stopping comparison closer than 1e-6"""
    X, y = S.dataset(data)
    est = S.reference(data, case)["est"]
    margins = []
    tw = S.twin_fit(X, y, order="sequential", margins=margins, **S.CASES[case])
    err = S.scaled_err(tw["coef"], tw["intercept"], est.coef_, est.intercept_)
    print("%s %s: n_iter %s, scaled error %.3g, closest stopping comparison %.3g" % (data, case, tw["n_iter"], err, min(margins)))
    assert max(tw["n_iter"]) == est.n_iter_ and tw["t"] == est.t_
    assert err <= 1e-14
    assert min(margins) >= 1e-6
    # the per-class epoch counts against one-problem fits of scikit-learn (n_iter_ is only their maximum)
    if len(tw["n_iter"]) > 1:
        assert len(set(tw["n_iter"])) > 1 or data != "main"
    # the kernel's order runs the same epochs
    assert S.reference(data, case)["kernel"]["n_iter"] == tw["n_iter"]


def test_cases_reach_the_rare_branches():
    """alpha = 10 reaches the wscale reset; alpha = 1e-8 reaches the outer log1pexp branches (|p| > 37)"""
    X, y = S.dataset("main")
    X64 = X.astype(np.float64)
    eta0 = 1.0 / (10.0 * S.optimal_init(10.0))
    assert max(0, 1.0 - eta0 * 10.0) < 1e-9                       # the first step's scale factor
    est = S.reference("main", "en_1e-8_avg")["est"]
    p = X64 @ est._standard_coef.T + est._standard_intercept
    assert p.max() > 33.3 and p.min() < -37


@pytest.mark.parametrize("n", [1, 2, 3, 97])
def test_shuffle_is_sklearns(T, n):
    from sklearn.utils._seq_dataset import ArrayDataset64
    small = next(s for s in range(1, 1 << 20) if S.our_rand_r(s)[1] < 4096)      # its first xorshift output is small
    for seed in (0, 1, 42, small, 2 ** 31 - 2, 2 ** 32 - 1):
        ds = ArrayDataset64(np.zeros((n, 1)), np.zeros(n), np.ones(n), seed=1)
        mine = np.arange(n, dtype=np.int32)
        twin = list(range(n))
        for _ in range(3):                                         # the permutations compound
            ds._shuffle_py(seed)
            mine = T.sgd_shuffle(seed, mine)
            S.shuffle_inplace(twin, seed)
            want = [ds._next_py()[3] for _ in range(n)]             # sample indices in the dataset's current order
            assert list(mine) == want and twin == want, (n, seed)


def test_seeds_are_sklearns(T):
    for nc in (2, 3, 5):
        assert T._sgd_seeds(7, nc) == S.shuffle_seeds(7, nc)


@pytest.fixture(scope="module")
def twin_search(T):
    gaps, calls = [], []
    old = T._sgd
    T._sgd = S.twin_hook("sequential", gaps, calls)
    try:
        X, y = S.search_rows()
        from sklearn.linear_model import SGDClassifier
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gs = T.GridSearchSGD(SGDClassifier(loss="log_loss", random_state=S.RANDOM_STATE), S.SEARCH_GRID, cv=S.SEARCH_CV).fit(X, y)
    finally:
        T._sgd = old
    return gs, gaps, calls


def test_search_logic(twin_search):
    gs, gaps, calls = twin_search
    ref = S.check_search(gs)
    assert len(calls) == 2                                         # ONE batch for the search, one more solve for the refit
    assert len(calls[0]["problems"]) == 4 * 3 * 3 and len(calls[0]["fits"]) == 12 and len(calls[1]["problems"]) == 3
    best, want = gs.best_estimator_, ref.best_estimator_
    assert S.scaled_err(best.coef_, best.intercept_, want.coef_, want.intercept_) <= 1e-14
    assert best.n_iter_ == want.n_iter_ and best.t_ == want.t_
    X, y = S.search_rows()
    np.testing.assert_array_equal(gs.predict(X), ref.predict(X.astype(np.float64)))


def test_search_fixture_is_valid(twin_search):
    """every held-out row's top-two decision gap is >= 1e-6, so the labels do not hang on the summation order"""
    _, gaps, _ = twin_search
    assert len(gaps) == 4 * 120 and min(gaps) >= 1e-6


@pytest.mark.parametrize("case", ["l2_1e-3", "en_1e-8_avg"])
@pytest.mark.parametrize("data", ["main", "bin"])
def test_fit_and_partial_fit_logic(T, monkeypatch, data, case):
    """fit_sgd, then partial_fit_sgd twice, with the twin as the device: the estimator scikit-learn builds, attribute for attribute"""
    from sklearn.linear_model import SGDClassifier
    monkeypatch.setattr(T, "_sgd", S.twin_hook("sequential"))
    X, y = S.dataset(data)
    kw = S.CASES[case]
    want = S.reference(data, case)["est"]
    got = T.fit_sgd(SGDClassifier(loss="log", max_iter=1000.0, random_state=S.RANDOM_STATE, **kw), X, y)
    assert got.loss == "log_loss" and got.max_iter == 1000
    names = ["coef_", "intercept_"] + (["_standard_coef", "_average_coef", "_standard_intercept", "_average_intercept"] if kw.get("average") else [])
    for name in names:
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-14 * np.abs(want.coef_).max(), name
    assert got.n_iter_ == want.n_iter_ and got.t_ == want.t_ and list(got.classes_) == list(want.classes_)
    assert got.n_features_in_ == want.n_features_in_
    np.testing.assert_array_equal(got.predict(X), want.predict(X.astype(np.float64)))
    assert got.predict_proba(X).shape == (len(y), len(want.classes_))
    a = SGDClassifier(loss="log_loss", random_state=S.RANDOM_STATE, **kw)
    b = SGDClassifier(loss="log_loss", random_state=S.RANDOM_STATE, **kw)
    half = len(y) // 2
    for sl in (slice(0, half), slice(half, None)):
        T.partial_fit_sgd(a, X[sl], y[sl], classes=np.unique(y))
        b.partial_fit(X[sl].astype(np.float64), y[sl], classes=np.unique(y))
        assert a.t_ == b.t_
        for name in names:
            u, v = getattr(a, name), getattr(b, name)
            assert u.shape == v.shape and np.abs(u - v).max() <= 1e-14 * np.abs(b.coef_).max(), name


def test_warnings_and_errors_as_sklearn(T, monkeypatch):
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import SGDClassifier
    monkeypatch.setattr(T, "_sgd", S.twin_hook("sequential"))
    X, y = S.dataset("bin")
    with pytest.warns(ConvergenceWarning, match="Maximum number of iteration reached"):
        T.fit_sgd(SGDClassifier(loss="log_loss", max_iter=2, random_state=0), X, y)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T.fit_sgd(SGDClassifier(loss="log_loss", max_iter=2, tol=None, random_state=0), X, y)      # tol=None never warns
    with pytest.raises(ValueError, match="classes must be passed"):
        T.partial_fit_sgd(SGDClassifier(loss="log_loss"), X, y)
    with pytest.raises(ValueError, match="balanced"):
        T.partial_fit_sgd(SGDClassifier(loss="log_loss", class_weight="balanced"), X, y, classes=[0, 1])


def test_unsupported_arguments_raise_before_device_work(T, monkeypatch):
    from sklearn.linear_model import SGDClassifier
    from sklearn.svm import SVC

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(T, "_sgd", no_device)
    X, y = S.dataset("bin")
    for kw in (dict(loss="hinge"), dict(learning_rate="constant", eta0=0.1), dict(early_stopping=True), dict(fit_intercept=False),
               dict(penalty=None)):
        est = SGDClassifier(**dict(dict(loss="log_loss"), **kw))
        with pytest.raises(NotImplementedError):
            T.fit_sgd(est, X, y)
        with pytest.raises(NotImplementedError):
            T.partial_fit_sgd(est, X, y, classes=[0, 1])
        with pytest.raises(NotImplementedError):
            T.GridSearchSGD(est, {"alpha": [1e-4]}, cv=2).fit(X, y)
    with pytest.raises(NotImplementedError):
        T.fit_sgd(SVC(), X, y)
    with pytest.raises(NotImplementedError):
        T.GridSearchSGD(SGDClassifier(loss="log_loss"), {"eta0": [0.1]}, cv=2).fit(X, y)
    with pytest.raises(NotImplementedError):
        T.GridSearchSGD(SGDClassifier(loss="log_loss"), {"alpha": [1e-4]}, cv=2, scoring="f1").fit(X, y)
    with pytest.raises(ValueError):
        T.fit_sgd(SGDClassifier(loss="log_loss", alpha=0.0), X, y)
    with pytest.raises(ValueError):
        T.fit_sgd(SGDClassifier(loss="log_loss"), X.astype(np.float64) + 1e-12, y)      # not float32-representable (_rows)
    with pytest.raises(ValueError):
        T.fit_sgd(SGDClassifier(loss="log_loss"), X, y[:-1])


def test_reference_grid(T, monkeypatch):
    """find_best_sgd_svm_estimator hands the reference's grid (35 candidates) and base estimator to GridSearchSGD"""
    seen = {}

    class Fake:
        def __init__(self, estimator, param_grid, **kw):
            seen.update(estimator=estimator, param_grid=param_grid, kw=kw)

        def fit(self, X, y):
            self.best_estimator_, self.best_score_, self.best_params_, self.n_splits_ = "est", 1.0, {}, 5
    monkeypatch.setattr(T, "GridSearchSGD", Fake)
    from sklearn.model_selection import ParameterGrid
    assert T.find_best_sgd_svm_estimator(np.zeros((500, 4), np.float32), np.zeros(500), 5, 1234) == "est"
    assert len(ParameterGrid(seen["param_grid"])) == 35
    p = seen["estimator"].get_params()
    assert p["loss"] == "log" and p["max_iter"] == 2000.0 and p["random_state"] == 1234 and p["warm_start"] is True


def test_option_and_header_in_step():
    from radar_ml_amd import _lib
    txt = open(os.path.join(ROOT, "include", "radarml.h")).read()
    assert int(re.search(r"#define\s+RML_OPT_SGD_RESIDENT_D\s+(\d+)", txt).group(1)) == _lib.option_id("sgd_resident_d")
    assert _lib.option_id("SGD_RESIDENT_D") == _lib.option_id("sgd_resident_d")
    assert int(re.search(r"#define\s+RML_SGD_RESIDENT_D_MAX\s+(\d+)", txt).group(1)) == _lib.SGD_RESIDENT_D_MAX
    assert int(re.search(r"#define\s+RML_SGD_MAX_ROWS\s+(\d+)", txt).group(1)) == _lib.SGD_MAX_ROWS
    assert _lib.ENV_OPTIONS["RML_SGD_RESIDENT_D"] == "sgd_resident_d"
    from radar_ml_amd import train as T
    assert T.SGD_PROBLEM.itemsize == 104 and T.SGD_FIT.itemsize == 16
