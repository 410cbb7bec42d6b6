"""ProjMaskSearchSVC without a GPU: the device hook (``radar_ml_amd.train._gram_masks``) replaced by a NumPy float64 segment-sum
Gram kept in the test helpers, the search checked against scikit-learn's GridSearchCV run live on every mask's column subset of
the real XY rows cut into three uneven segments."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
import mask_search_common as M  # noqa: E402
sys.path.pop(0)


@pytest.fixture(scope="module")
def T():
    import radar_ml_amd.train as T
    return T


@pytest.fixture
def numpy_hook(T, monkeypatch):
    class Calls(list):
        segments = []
    calls = Calls()

    def hook(X, segments, keys, device=None):
        assert X.dtype == np.float32 and X.flags.c_contiguous and sum(segments) == X.shape[1]
        calls.append(list(keys))
        calls.segments.append(tuple(segments))
        return M.numpy_gram_masks(X, segments, keys, device)
    monkeypatch.setattr(T, "_gram_masks", hook)

    def no_device(*a, **k):
        raise AssertionError("the mask search went to another device hook")
    for name in ("_gram", "_smo", "_smo_masks"):
        monkeypatch.setattr(T, name, no_device)
    return calls


def search(T, grid, **kw):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    return T.ProjMaskSearchSVC(G.base_svc(), grid, M.SEGMENTS, cv=StratifiedKFold(5).split(X, y), n_jobs=4, **kw).fit(X, y)


def test_sub_grid_every_mask_matches_gridsearchcv(T, numpy_hook):
    from radar_ml_amd import ProjMask
    ours = search(T, M.SUB_GRID)
    mask, ref = M.check_scores(ours, "sub")
    assert ours.best_proj_mask_ == ProjMask(xz=False, yz=True, xy=True)
    assert ours.best_params_ == {"C": 10, "kernel": "linear"}
    assert ours.best_score_ == ref.best_score_ == 0.841125541125541
    assert set(ours.cv_results_) == set(ref.cv_results_) | {"param_proj_mask"}
    # 7 masks x (linear + two gammas) in one hook call; the refit reuses the winner's matrix
    assert len(numpy_hook) == 1 and len(numpy_hook[0]) == 21
    assert numpy_hook[0][0] == (1, "linear", None) and numpy_hook[0][-1] == (7, "rbf", 0.1)


def test_reference_grid_winner_and_estimator(T, numpy_hook):
    from radar_ml_amd import ProjMask
    X, y = G.real_xy()
    ours = search(T, G.GRID)
    mask, ref = M.check_scores(ours, "full")
    assert ours.best_proj_mask_ == ProjMask(True, False, False)
    assert ours.best_params_ == {"C": 0.1, "gamma": 1, "kernel": "rbf"}
    assert len(numpy_hook) == 1 and len(numpy_hook[0]) == 42
    # best_estimator_ against the live winner's, under the bounds of grid_search_common.check_parity
    Xm = np.ascontiguousarray(X[:, M.cols_of(mask)])
    be, re_ = ours.best_estimator_, ref.best_estimator_
    assert type(be) is type(re_) and be.get_params() == re_.get_params()
    va, vb = vars(be), vars(re_)
    assert set(va) == set(vb)
    for k, v in vb.items():
        if isinstance(v, np.ndarray):
            assert isinstance(va[k], np.ndarray) and va[k].shape == v.shape and va[k].dtype == v.dtype, k
        else:
            assert type(va[k]) is type(v), k
    assert be.shape_fit_ == re_.shape_fit_ and be.n_features_in_ == re_.n_features_in_ == M.SEGMENTS[0]
    assert be._gamma == re_._gamma
    assert np.array_equal(be.support_vectors_, Xm.astype(np.float64)[be.support_])
    assert np.abs(be.decision_function(Xm) - re_.decision_function(Xm)).max() <= 2e-3
    assert np.abs(be.predict_proba(Xm) - re_.predict_proba(Xm)).max() <= 5e-3
    assert np.array_equal(be.predict(Xm), re_.predict(Xm))
    blob = pickle.dumps(be)
    assert b"radar_ml_amd" not in blob and b"radar-ml_amd" not in blob
    assert np.array_equal(pickle.loads(blob).predict(Xm), be.predict(Xm))
    assert ours.refit_time_ > 0


def test_groups_respect_max_gram_bytes(T, numpy_hook):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    X, y = X[:120], y[:120]
    grid = {"C": [1.0], "gamma": [0.01, 0.1], "kernel": ["rbf"]}
    mk = lambda **kw: T.ProjMaskSearchSVC(G.base_svc(), grid, M.SEGMENTS, cv=StratifiedKFold(3), **kw).fit(X, y)
    one = mk()
    assert [len(c) for c in numpy_hook] == [14]
    numpy_hook.clear()
    small = mk(max_gram_bytes=4 * 120 * 120 * 8)
    assert [len(c) for c in numpy_hook[:4]] == [4, 4, 4, 2]
    assert sum(numpy_hook[:4], []) == [(b, "rbf", g) for b in range(1, 8) for g in (0.01, 0.1)]
    for key in M.SCORE_KEYS[:3] + M.SCORE_KEYS[5:] + ["rank_test_score"]:
        assert np.array_equal(small.cv_results_[key], one.cv_results_[key]), key
    assert small.best_proj_mask_ == one.best_proj_mask_ and small.best_params_ == one.best_params_
    assert np.array_equal(small.best_estimator_.dual_coef_, one.best_estimator_.dual_coef_)
    numpy_hook.clear()
    with pytest.raises(ValueError, match="max_gram_bytes"):
        mk(max_gram_bytes=1000)
    assert numpy_hook == []


def test_masks_subset_order_and_ties(T, numpy_hook):
    from radar_ml_amd import ProjMask
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    xy, yz_xy = ProjMask(False, False, True), ProjMask(False, True, True)
    masks = [xy, yz_xy, xy, yz_xy]
    ours = T.ProjMaskSearchSVC(G.base_svc(), M.SUB_GRID, M.SEGMENTS, proj_masks=masks, cv=StratifiedKFold(5)).fit(X, y)
    per = 6
    assert [p["proj_mask"] for p in ours.cv_results_["params"]] == [m for m in masks for _ in range(per)]
    live = M.live_searches("sub")
    for mi, m in enumerate(masks):
        ref = live[M.all_masks().index(m)]
        assert np.array_equal(ours.cv_results_["mean_test_score"][mi * per:(mi + 1) * per], ref.cv_results_["mean_test_score"])
    # yz + xy wins (0.8411 over xy's best); its FIRST occurrence is the winner, and the duplicates share rank 1
    assert ours.best_proj_mask_ == yz_xy and ours.best_index_ == per + live[5].best_index_
    assert ours.cv_results_["rank_test_score"][ours.best_index_ + 2 * per] == 1
    assert len(numpy_hook) == 1 and len(numpy_hook[0]) == 6          # two distinct masks x three kernels
    cols = M.cols_of(yz_xy)
    assert ours.best_estimator_.n_features_in_ == len(cols)
    assert np.array_equal(ours.predict(X), ours.best_estimator_.predict(X[:, cols]))
    assert np.array_equal(ours.decision_function(X), ours.best_estimator_.decision_function(X[:, cols]))
    assert np.array_equal(ours.predict_proba(X), ours.best_estimator_.predict_proba(X[:, cols]))
    assert ours.score(X, y) == ours.best_estimator_.score(X[:, cols], y)
    with pytest.raises(ValueError, match="full rows"):
        ours.predict(X[:, cols])


def test_bad_arguments_raise(T, numpy_hook):
    from radar_ml_amd import ProjMask
    X, y = G.real_xy()
    X, y = X[:60], y[:60]
    grid = {"C": [1.0], "kernel": ["linear"]}
    with pytest.raises(ValueError, match="segments"):
        T.ProjMaskSearchSVC(G.base_svc(), grid, (264, 372, 47)).fit(X, y)
    with pytest.raises(ValueError, match="segments"):
        T.ProjMaskSearchSVC(G.base_svc(), grid, (264, 418)).fit(X, y)
    with pytest.raises(ValueError, match="zero length"):
        T.ProjMaskSearchSVC(G.base_svc(), grid, (0, 636, 46), proj_masks=[ProjMask(True, True, False)]).fit(X, y)
    with pytest.raises(ValueError, match="zero length"):
        T.ProjMaskSearchSVC(G.base_svc(), grid, (0, 636, 46)).fit(X, y)          # the default masks include xz
    with pytest.raises(ValueError, match="no projection"):
        T.ProjMaskSearchSVC(G.base_svc(), grid, M.SEGMENTS, proj_masks=[ProjMask(False, False, False)]).fit(X, y)
    # GridSearchSVC's refusals carry over
    for bad in ({"kernel": ["poly"]}, {"C": [1.0], "gamma": ["scale"], "kernel": ["rbf"]}, {"degree": [2], "kernel": ["rbf"]}):
        with pytest.raises(NotImplementedError):
            T.ProjMaskSearchSVC(G.base_svc(), bad, M.SEGMENTS).fit(X, y)
    with pytest.raises(NotImplementedError):
        T.ProjMaskSearchSVC(G.base_svc(), grid, M.SEGMENTS, scoring="f1").fit(X, y)
    with pytest.raises(ValueError, match="solver"):
        T.ProjMaskSearchSVC(G.base_svc(), grid, M.SEGMENTS, solver="gpu").fit(X, y)
    with pytest.raises(ValueError, match="C must be > 0"):
        T.ProjMaskSearchSVC(G.base_svc(), {"C": [0.0], "kernel": ["linear"]}, M.SEGMENTS).fit(X, y)
    assert numpy_hook == []                     # every refusal comes before any device work
    # a zero-length segment that no mask selects is fine
    ok = T.ProjMaskSearchSVC(G.base_svc(), grid, (0, 636, 46), proj_masks=[ProjMask(False, True, True)], cv=3)
    ok.fit(X, y)
    assert numpy_hook.segments == [(0, 636, 46)] and numpy_hook == [[(6, "linear", None)]]
    assert ok.best_estimator_.n_features_in_ == 682


def test_exports_and_reference_call(T, numpy_hook):
    import radar_ml_amd as R
    from sklearn.model_selection import StratifiedKFold
    assert R.ProjMaskSearchSVC is T.ProjMaskSearchSVC and R.svc_fit_masks is T.svc_fit_masks
    assert R.find_best_proj_mask_svm_estimator is T.find_best_proj_mask_svm_estimator
    for name in ("ProjMaskSearchSVC", "find_best_proj_mask_svm_estimator", "svc_fit_masks"):
        assert name in R.__all__
    X, y = G.real_xy()
    masks = [R.ProjMask(True, False, False), R.ProjMask(False, False, True)]
    est, mask = T.find_best_proj_mask_svm_estimator(X, y, StratifiedKFold(5).split(X, y), G.SEED, M.SEGMENTS, proj_masks=masks)
    ref = M.live_searches("full")[0]
    assert mask == R.ProjMask(True, False, False) and type(est).__name__ == "SVC"
    assert est.get_params() == ref.best_estimator_.get_params() and est.n_features_in_ == M.SEGMENTS[0]
    assert len(numpy_hook) == 1 and len(numpy_hook[0]) == 12
