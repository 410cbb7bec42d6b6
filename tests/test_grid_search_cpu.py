"""GridSearchSVC without a GPU: the device hook (``radar_ml_amd.train._gram``) replaced by a NumPy float64 Gram kept in the test
helpers, the search logic checked against scikit-learn's GridSearchCV run live on the reference's grid and the real XY rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
sys.path.pop(0)


@pytest.fixture(scope="module")
def T():
    import radar_ml_amd.train as T
    return T


@pytest.fixture
def numpy_hook(T, monkeypatch):
    calls = []

    def hook(X, kernels, device=None):
        assert X.dtype == np.float32 and X.flags.c_contiguous and 1 <= len(kernels) <= 8
        calls.append(list(kernels))
        return G.numpy_gram(X, kernels, device)
    monkeypatch.setattr(T, "_gram", hook)
    return calls


@pytest.fixture(scope="module")
def searched(T):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "_gram", G.numpy_gram)
        ours = T.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4).fit(X, y)
    return X, y, ours, G.sklearn_search(X, y)


def test_reference_grid_matches_gridsearchcv(searched):
    X, y, ours, ref = searched
    G.check_parity(ours, ref, X, y)
    assert ours.refit_time_ > 0 and ours.scorer_ is not None


def test_find_best_svm_estimator_is_the_reference_call(T, numpy_hook, searched):
    from sklearn.model_selection import StratifiedKFold
    X, y, ours, _ = searched
    best = T.find_best_svm_estimator(X, y, StratifiedKFold(5).split(X, y), G.SEED)
    assert type(best).__name__ == "SVC" and best.get_params() == ours.best_estimator_.get_params()
    assert np.array_equal(best.dual_coef_, ours.best_estimator_.dual_coef_)
    # six distinct kernels (linear + five gammas) in one Gram call; the refit reuses its matrix
    assert len(numpy_hook) == 1 and len(numpy_hook[0]) == 6


def test_cv_forms_agree(T, numpy_hook):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    X, y = X[::2], y[::2]
    grid = [{"C": [0.1, 10], "kernel": ["linear"]}, {"C": [1, 100], "gamma": [0.01, 1.0], "kernel": ["rbf"]}]
    runs = [T.GridSearchSVC(G.base_svc(), grid, cv=cv, n_jobs=2).fit(X, y)
            for cv in (3, StratifiedKFold(3), StratifiedKFold(3).split(X, y))]
    for r in runs[1:]:
        assert r.n_splits_ == 3 and r.best_params_ == runs[0].best_params_
        for k in range(3):
            assert np.array_equal(r.cv_results_["split%d_test_score" % k], runs[0].cv_results_["split%d_test_score" % k])


def test_gram_groups_respect_max_gram_bytes(T, numpy_hook):
    X, y = G.real_xy()
    X, y = X[:120], y[:120]
    grid = {"C": [1.0], "gamma": [0.001, 0.01, 0.1, 1.0, 10.0], "kernel": ["rbf"]}
    one = T.GridSearchSVC(G.base_svc(), grid, cv=3).fit(X, y)
    numpy_hook.clear()
    small = T.GridSearchSVC(G.base_svc(), grid, cv=3, max_gram_bytes=2 * 120 * 120 * 8).fit(X, y)
    assert [len(c) for c in numpy_hook[:3]] == [2, 2, 1]
    assert np.array_equal(small.cv_results_["mean_test_score"], one.cv_results_["mean_test_score"])
    with pytest.raises(ValueError, match="max_gram_bytes"):
        T.GridSearchSVC(G.base_svc(), grid, cv=3, max_gram_bytes=1000).fit(X, y)


def test_out_of_range_raises(T, numpy_hook):
    from sklearn.svm import SVC
    X, y = G.real_xy()
    X, y = X[:60], y[:60]
    for grid in ({"kernel": ["poly"]}, {"kernel": ["sigmoid"]}, {"C": [1.0], "gamma": ["scale"], "kernel": ["rbf"]},
                 {"C": [1.0], "gamma": ["auto"], "kernel": ["rbf"]}, {"C": [1.0]}, {"degree": [2], "kernel": ["rbf"]}):
        with pytest.raises(NotImplementedError):
            T.GridSearchSVC(G.base_svc(), grid).fit(X, y)
    grid = {"C": [1.0], "kernel": ["linear"]}
    with pytest.raises(NotImplementedError):
        T.GridSearchSVC(G.base_svc(), grid, scoring="f1").fit(X, y)
    with pytest.raises(NotImplementedError):
        T.GridSearchSVC(G.base_svc(), grid, refit=lambda r: 0).fit(X, y)
    with pytest.raises(NotImplementedError):
        T.GridSearchSVC(SVC(kernel="poly"), {"C": [1.0]}).fit(X, y)
    assert numpy_hook == []                     # every refusal comes before any device work


def test_bad_rows_raise(T, numpy_hook):
    X, y = G.real_xy()
    X, y = X[:60], y[:60]
    grid = {"C": [1.0], "kernel": ["linear"]}
    with pytest.raises(ValueError, match="float32"):
        T.GridSearchSVC(G.base_svc(), grid).fit(X.astype(np.float64) + 1e-12, y)
    with pytest.raises(ValueError, match="Expected 2D array"):
        T.GridSearchSVC(G.base_svc(), grid).fit(X[0], y)
    bad = X.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="Input contains NaN"):
        T.GridSearchSVC(G.base_svc(), grid).fit(bad, y)
    bad[3, 5] = np.inf
    with pytest.raises(ValueError, match="Input contains NaN"):
        T.GridSearchSVC(G.base_svc(), grid).fit(bad, y)
    with pytest.raises(ValueError, match="gamma"):
        T.GridSearchSVC(G.base_svc(), {"C": [1.0], "gamma": [-1.0], "kernel": ["rbf"]}).fit(X, y)
    with pytest.raises(ValueError, match="inconsistent"):
        T.GridSearchSVC(G.base_svc(), grid).fit(X, y[:-1])
    assert numpy_hook == []
    # float64 rows that ARE float32 values are accepted and give the float32 search
    a = T.GridSearchSVC(G.base_svc(), grid, cv=3).fit(X.astype(np.float64), y)
    b = T.GridSearchSVC(G.base_svc(), grid, cv=3).fit(X, y)
    assert np.array_equal(a.best_estimator_.dual_coef_, b.best_estimator_.dual_coef_)


def test_package_exports():
    import radar_ml_amd
    assert radar_ml_amd.GridSearchSVC is radar_ml_amd.train.GridSearchSVC
    assert radar_ml_amd.find_best_svm_estimator is radar_ml_amd.train.find_best_svm_estimator


def test_progress_lines_and_n_jobs_convention(T, numpy_hook, capsys):
    """verbose=2 prints GridSearchCV's header and one line per fit (train.py:485 passes verbose=2); n_jobs follows joblib's
    convention (-1: every CPU the process may use, -2: all but one), never more threads than fits"""
    X, y = G.real_xy()
    X, y = X[:90], y[:90]
    grid = [{"C": [1.0], "kernel": ["linear"]}, {"C": [10.0], "gamma": [0.01], "kernel": ["rbf"]}]
    ref = T.GridSearchSVC(G.base_svc(), grid, cv=3, n_jobs=1).fit(X, y)
    capsys.readouterr()
    for nj in (-1, -2, None, 64):
        r = T.GridSearchSVC(G.base_svc(), grid, cv=3, n_jobs=nj, verbose=2).fit(X, y)
        assert np.array_equal(r.cv_results_["mean_test_score"], ref.cv_results_["mean_test_score"])
        out = capsys.readouterr().out.splitlines()
        assert out[0] == "Fitting 3 folds for each of 2 candidates, totalling 6 fits"
        assert len([line for line in out if line.startswith("[CV ") and " END C=" in line]) == 6
