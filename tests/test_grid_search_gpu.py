"""GridSearchSVC on the real rml_gram: the reference's grid on the real XY rows against a live GridSearchCV, the winner through
from_sklearn and the calibration step of train.py:722-724, and an off-grid search at the reference's feature length."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
sys.path.pop(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def searched(rml):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    ours = rml.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4).fit(X, y)
    return X, y, ours, G.sklearn_search(X, y)


def test_reference_grid_on_gpu_gram_matches_gridsearchcv(searched):
    X, y, ours, ref = searched
    G.check_parity(ours, ref, X, y)


def test_winner_through_from_sklearn_and_calibration(rml, searched):
    from sklearn.calibration import CalibratedClassifierCV
    X, y, ours, _ = searched
    clf = ours.best_estimator_
    gpu = rml.from_sklearn(clf)
    assert np.abs(gpu.decision_function(X) - clf.decision_function(X)).max() <= 1e-5
    assert np.array_equal(gpu.predict(X), clf.predict(X))
    # train.py:722-724 on the result: CalibratedClassifierCV(prefit) on held-out rows, then the GPU twin of the calibrated model
    val = np.arange(len(y)) % 4 == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # cv='prefit' is deprecated in scikit-learn 1.6+; the reference uses it
        cal = CalibratedClassifierCV(estimator=clf, cv="prefit").fit(X[val], y[val])
    gcal = rml.from_sklearn(cal)
    assert np.array_equal(gcal.predict(X), cal.predict(X))
    assert np.abs(gcal.predict_proba(X) - cal.predict_proba(X)).max() <= 1e-5


def test_off_grid_rows_at_reference_feature_length(rml):
    """a seeded off-grid set at D = 10 010 (the reference's three planes), linear + 2 C x 2 gamma: live GridSearchCV agrees"""
    rng = np.random.default_rng(20)
    N, D = 300, 10010
    y = np.arange(N) % 3
    centers = 0.5 + 0.03 * rng.standard_normal((3, D))
    X = np.clip(centers[y] + 0.25 * rng.standard_normal((N, D)), 0.0, 1.0).astype(np.float32)
    grid = [{"C": [0.1, 10], "kernel": ["linear"]}, {"C": [1, 100], "gamma": [1e-4, 1e-3], "kernel": ["rbf"]}]
    ours = rml.GridSearchSVC(G.base_svc(), grid, cv=5, n_jobs=4).fit(X, y)
    ref = G.sklearn_search(X, y, grid)
    assert ours.best_params_ == ref.best_params_
    for k in range(5):
        key = "split%d_test_score" % k
        assert np.array_equal(ours.cv_results_[key], ref.cv_results_[key]), key
    assert np.array_equal(ours.best_estimator_.predict(X), ref.best_estimator_.predict(X))
