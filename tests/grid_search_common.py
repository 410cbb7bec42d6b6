"""Shared checks of the SVC grid search (tests/test_grid_search_cpu.py, tests/test_grid_search_gpu.py): the reference's grid on the
real XY fixture, GridSearchSVC against scikit-learn's own GridSearchCV run live on the same rows."""
import os
import pickle

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 1234
CS = [0.01, 0.1, 1, 10, 100]
GAMMAS = [0.001, 0.01, 0.1, 1, 10]
GRID = [{"C": CS, "kernel": ["linear"]}, {"C": CS, "gamma": GAMMAS, "kernel": ["rbf"]}]     # train.py:477-481


def real_xy():
    """491 rows x 682 (the xy plane of the real captures), float32(c/255) like train.py:667 gives them to scikit-learn."""
    g = np.load(os.path.join(GOLDEN, "real_xy_svm.npz"))
    X = (g["xy_u8"].reshape(len(g["labels"]), -1).astype(np.float32) / np.float32(255.0))
    return X, g["labels"].astype(np.int64)


def base_svc():
    from sklearn import svm
    return svm.SVC(probability=True, class_weight="balanced", random_state=SEED, cache_size=1000, verbose=False)   # train.py:482-483


def numpy_gram(X, kernels, device=None):
    """float64 NumPy twin of rml_gram (test oracle only: the package ships no host Gram)."""
    X64 = np.asarray(X, dtype=np.float64)
    dot = X64 @ X64.T
    sq = (X64 * X64).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * dot
    return [dot.copy() if k == "linear" else np.exp(-g * d2) for k, g in kernels]


def sklearn_search(X, y, grid=GRID, n_jobs=4):
    from sklearn import model_selection
    gs = model_selection.GridSearchCV(base_svc(), grid, n_jobs=n_jobs, cv=model_selection.StratifiedKFold(5).split(X, y))
    return gs.fit(X, y)


def check_parity(ours, ref, X, y):
    """Everything the search promises against a live GridSearchCV on the same rows."""
    assert ours.best_params_ == ref.best_params_
    assert ours.best_score_ == ref.best_score_
    assert ours.best_index_ == ref.best_index_
    assert ours.n_splits_ == ref.n_splits_
    assert set(ours.cv_results_) == set(ref.cv_results_)
    assert ours.cv_results_["params"] == ref.cv_results_["params"]
    for k in range(ref.n_splits_):
        key = "split%d_test_score" % k
        assert np.array_equal(ours.cv_results_[key], ref.cv_results_[key]), key
    for key in ("mean_test_score", "std_test_score", "rank_test_score"):
        assert np.array_equal(ours.cv_results_[key], ref.cv_results_[key]), key
        assert ours.cv_results_[key].dtype == ref.cv_results_[key].dtype, key
    for key in [k for k in ref.cv_results_ if k.startswith("param_")]:
        a, b = ours.cv_results_[key], ref.cv_results_[key]
        assert isinstance(a, np.ma.MaskedArray) and a.dtype == b.dtype, key
        assert np.array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b)), key
        assert list(a.compressed()) == list(b.compressed()), key
    linear = np.array([p["kernel"] == "linear" for p in ref.cv_results_["params"]])
    assert np.ma.getmaskarray(ours.cv_results_["param_gamma"])[linear].all()

    be, re_ = ours.best_estimator_, ref.best_estimator_
    assert type(be) is type(re_)
    assert be.get_params() == re_.get_params()
    va, vb = vars(be), vars(re_)
    assert set(va) == set(vb)
    for k, v in vb.items():
        if isinstance(v, np.ndarray):
            assert isinstance(va[k], np.ndarray) and va[k].shape == v.shape and va[k].dtype == v.dtype, k
        else:
            assert type(va[k]) is type(v), k
    assert be.shape_fit_ == re_.shape_fit_ and be.n_features_in_ == re_.n_features_in_
    assert be._gamma == re_._gamma
    assert np.array_equal(be.support_vectors_, X.astype(np.float64)[be.support_])
    assert np.abs(be.decision_function(X) - re_.decision_function(X)).max() <= 2e-3
    assert np.abs(be.predict_proba(X) - re_.predict_proba(X)).max() <= 5e-3
    assert np.array_equal(be.predict(X), re_.predict(X))
    blob = pickle.dumps(be)
    assert b"radar_ml_amd" not in blob and b"radar-ml_amd" not in blob
    assert np.array_equal(pickle.loads(blob).predict(X), be.predict(X))
