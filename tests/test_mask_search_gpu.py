"""ProjMaskSearchSVC on the real rml_gram_segments / rml_gram_compose: the host, device and device-refit routes on the real XY rows
cut into three segments against scikit-learn's GridSearchCV run live on every mask's column subset, and ``svc_fit_masks`` on a
small synthetic set of projection tuples."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
import mask_search_common as M  # noqa: E402
sys.path.pop(0)

pytestmark = pytest.mark.gpu

ROUTES = {"host": dict(solver="host"), "device": dict(solver="device"), "device-refit": dict(solver="device", refit_solver="device")}


def fit(rml, **kw):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    return rml.ProjMaskSearchSVC(G.base_svc(), M.SUB_GRID, M.SEGMENTS, cv=StratifiedKFold(5).split(X, y), n_jobs=4, **kw).fit(X, y)


@pytest.fixture(scope="module")
def routes(rml):
    return {name: fit(rml, **kw) for name, kw in ROUTES.items()}


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_matches_gridsearchcv_on_every_mask(rml, routes, route):
    ours = routes[route]
    mask, ref = M.check_scores(ours, "sub")
    assert mask == rml.ProjMask(xz=False, yz=True, xy=True) and ours.best_params_ == {"C": 10, "kernel": "linear"}
    X, _ = G.real_xy()
    Xm = np.ascontiguousarray(X[:, M.cols_of(mask)])
    be, re_ = ours.best_estimator_, ref.best_estimator_
    assert type(be) is type(re_) and be.get_params() == re_.get_params() and be.n_features_in_ == Xm.shape[1]
    assert np.array_equal(be.support_vectors_, Xm.astype(np.float64)[be.support_])
    assert np.abs(be.decision_function(Xm) - re_.decision_function(Xm)).max() <= 2e-3
    assert np.abs(be.predict_proba(Xm) - re_.predict_proba(Xm)).max() <= 5e-3
    assert np.array_equal(ours.predict(X), re_.predict(Xm))


def test_host_and_device_routes_agree(routes):
    host = routes["host"]
    for name in ("device", "device-refit"):
        dev = routes[name]
        for key in M.SCORE_KEYS + ["rank_test_score"]:
            assert np.array_equal(dev.cv_results_[key], host.cv_results_[key]), (name, key)
        # both see the same composed matrix
        assert np.array_equal(dev.best_estimator_.dual_coef_, host.best_estimator_.dual_coef_), name
        assert np.array_equal(dev.best_estimator_.intercept_, host.best_estimator_.intercept_), name
        assert np.array_equal(dev.best_estimator_.support_, host.best_estimator_.support_), name


def test_second_fit_gives_the_same_bits(rml, routes):
    again = fit(rml, **ROUTES["device-refit"])
    first = routes["device-refit"]
    for key in M.SCORE_KEYS:
        assert np.array_equal(again.cv_results_[key], first.cv_results_[key]), key
    for attr in ("dual_coef_", "intercept_", "support_", "probA_", "probB_"):
        assert np.array_equal(getattr(again.best_estimator_, attr), getattr(first.best_estimator_, attr)), attr


def test_no_kernel_matrix_comes_back_with_device_refit(rml, monkeypatch):
    import radar_ml_amd.train as T
    real = T._smo_masks
    fetched = []

    def watched(X, segments, keys, plan, device=None):
        out = real(X, segments, keys, plan, device)
        m = out["matrix"]
        out["matrix"] = lambda k: (fetched.append(k), m(k))[1]
        return out
    monkeypatch.setattr(T, "_smo_masks", watched)
    monkeypatch.setattr(T, "_gram_masks", lambda *a, **k: pytest.fail("a host copy of the matrices was asked for"))
    fit(rml, **ROUTES["device-refit"])
    assert fetched == []


def test_svc_fit_masks_picks_the_separable_plane(rml):
    """~120 projection tuples, three classes that differ in the yz plane only (xz and xy are noise)"""
    import radar_ml_amd.train as T
    from sklearn.svm import SVC
    rng = np.random.default_rng(5)
    shapes = ((8, 16), (10, 16), (8, 10))                              # xz, yz, xy of an (X, Y, Z) = (8, 10, 16) volume
    n = 120
    y = (np.arange(n) % 3).astype(np.int8)
    pattern = rng.random((3,) + shapes[1])
    samples = []
    for c in y:
        yz = np.clip(0.5 + 0.3 * (pattern[c] - 0.5) + 0.05 * rng.standard_normal(shapes[1]), 0.0, 1.0)
        samples.append((rng.random(shapes[0]).astype(np.float32), yz.astype(np.float32), rng.random(shapes[2]).astype(np.float32)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf, mask = T.svc_fit_masks((samples, y), epochs=0, solver="device", refit_solver="device")
    assert mask == rml.ProjMask(xz=False, yz=True, xy=False)
    assert type(clf) is SVC and clf.n_features_in_ == 160
    rows = np.asarray(rml.process_samples(samples, proj_mask=mask))
    assert rows.shape == (n, 160) and np.array_equal(clf.predict(rows), y)
