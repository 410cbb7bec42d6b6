"""The device SVC solver without a GPU: the NumPy twin of libsvm's solver (tests/smo_common.py) against scikit-learn run live, bit
for bit, and GridSearchSVC(solver="device") with both device hooks (``train._gram``, ``train._smo``) replaced by their twins."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
import smo_common as S  # noqa: E402
sys.path.pop(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import radar_ml_amd.train as T
    return T


def _twin_case(prob, **kw):
    alpha, rho, it, nshr, stopped = S.twin_solve(prob, **kw)
    S.check_against_sklearn(prob, alpha, rho, it, **kw)
    return it, nshr, stopped


@pytest.mark.parametrize("k", range(len(S.REAL_KERNELS)))
def test_twin_is_libsvm_on_real_xy_pairs(k):
    """n_iter, support set, alpha and rho of SVC(kernel='precomputed').fit, bit for bit, on the three class pairs of one kernel"""
    for prob in S.real_problems()[3 * k:3 * k + 3]:
        _twin_case(prob)


def test_twin_shrinks_and_reconstructs():
    """the fixture does exercise the shrinking and reconstruction paths"""
    prob = S.real_problems()[3 + 2]                 # linear C = 10, the 469-row pair
    it, nshr, _ = _twin_case(prob)
    assert it > 1000 and nshr >= 2
    it2, nshr2, _ = _twin_case(prob, shrinking=False)
    assert nshr2 == 0


def test_twin_early_stop():
    for prob in S.real_problems()[3:6]:
        it, _, stopped = _twin_case(prob, max_iter=50)
        assert it == 50 and stopped


def test_twin_early_stop_after_shrinking():
    """stopped with active_size < l: after the first shrink pass of the 469-row dual (counter = l + 1)"""
    it, nshr, stopped = _twin_case(S.real_problems()[5], max_iter=600)
    assert it == 600 and stopped and nshr >= 1


def test_twin_past_1000_rows():
    for prob in S.big_problems():
        it, nshr, _ = _twin_case(prob)
        assert nshr >= 2


def test_twin_degenerate():
    copies, two = S.degenerate_problems()
    assert _twin_case(copies)[0] == 6
    assert _twin_case(two)[0] == 1


@pytest.fixture(scope="module")
def searched(T):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    calls = []

    def smo(Xh, kernels, plan, device=None):
        assert Xh.dtype == np.float32 and plan["problems"].dtype == T.SMO_PROBLEM and plan["fits"].dtype == T.SMO_FIT
        calls.append((list(kernels), len(plan["problems"]), len(plan["fits"])))
        return S.twin_smo(Xh, kernels, plan, device)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "_gram", G.numpy_gram)
        mp.setattr(T, "_smo", smo)
        dev = T.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4, solver="device").fit(X, y)
        host = T.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4, solver="host").fit(X, y)
    return X, y, dev, host, calls


def test_device_search_matches_gridsearchcv(searched):
    X, y, dev, _, calls = searched
    G.check_parity(dev, G.sklearn_search(X, y), X, y)
    # one group of six kernels: ONE batched call with 30 candidates x 5 splits fits of 3 class pairs each
    assert [(len(k), p, f) for k, p, f in calls] == [(6, 450, 150)]


def test_device_split_scores_equal_host(searched):
    _, _, dev, host, _ = searched
    for k in range(5):
        key = "split%d_test_score" % k
        assert np.array_equal(dev.cv_results_[key], host.cv_results_[key]), key
    assert dev.best_params_ == host.best_params_
    assert np.array_equal(dev.best_estimator_.dual_coef_, host.best_estimator_.dual_coef_)
    # the batch's time divided evenly among its fits
    assert len(set(dev.cv_results_["mean_fit_time"])) == 1 and dev.cv_results_["mean_fit_time"][0] > 0


def test_fold_without_a_class_takes_the_host_path(T, monkeypatch):
    """a split whose training rows miss a class is libsvm's business: that fit runs on the host, the others on the device"""
    X, y = G.real_xy()
    keep = np.concatenate([np.nonzero(y == 0)[0][:20], np.nonzero(y == 1)[0][:20], np.nonzero(y == 2)[0][:2]])
    X, y = X[keep], y[keep]
    idx = np.arange(len(y))
    last = idx[y == 2]
    splits = [(np.setdiff1d(idx, te), te) for te in (np.concatenate([idx[:5], idx[20:25]]), np.concatenate([idx[5:10], last]))]
    seen = []
    monkeypatch.setattr(T, "_gram", G.numpy_gram)
    monkeypatch.setattr(T, "_smo", lambda Xh, ks, plan, device=None: (seen.append(len(plan["fits"])), S.twin_smo(Xh, ks, plan))[1])
    grid = {"C": [1.0, 10.0], "kernel": ["linear"]}
    dev = T.GridSearchSVC(G.base_svc(), grid, cv=splits, solver="device").fit(X, y)
    host = T.GridSearchSVC(G.base_svc(), grid, cv=splits, solver="host").fit(X, y)
    assert seen == [2]                              # split 0 of both candidates on the device, split 1 on the host
    for k in range(2):
        assert np.array_equal(dev.cv_results_["split%d_test_score" % k], host.cv_results_["split%d_test_score" % k])


def test_base_estimator_settings_reach_the_plan(T, monkeypatch):
    from sklearn.svm import SVC
    X, y = G.real_xy()
    X, y = X[::4], y[::4]
    plans = []
    monkeypatch.setattr(T, "_gram", G.numpy_gram)
    monkeypatch.setattr(T, "_smo", lambda Xh, ks, plan, device=None: (plans.append(plan), S.twin_smo(Xh, ks, plan))[1])
    base = SVC(class_weight={0: 2.0, 1: 1.0, 2: 0.5}, tol=1e-2, shrinking=False, max_iter=40)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = T.GridSearchSVC(base, {"C": [3.0], "kernel": ["linear"]}, cv=3, solver="device").fit(X, y)
        host = T.GridSearchSVC(base, {"C": [3.0], "kernel": ["linear"]}, cv=3, solver="host").fit(X, y)
    pr = plans[0]["problems"]
    assert set(pr["eps"]) == {1e-2} and set(pr["shrinking"]) == {0} and set(pr["max_iter"]) == {40}
    assert list(pr["Cp"][:3]) == [6.0, 6.0, 3.0] and list(pr["Cn"][:3]) == [3.0, 1.5, 1.5]
    for k in range(3):
        assert np.array_equal(dev.cv_results_["split%d_test_score" % k], host.cv_results_["split%d_test_score" % k])


def test_unknown_solver_raises(T):
    X, y = G.real_xy()
    with pytest.raises(ValueError, match="solver"):
        T.GridSearchSVC(G.base_svc(), G.GRID, solver="bogus").fit(X[:60], y[:60])
    with pytest.raises(ValueError, match="solver"):
        T.find_best_svm_estimator(X[:60], y[:60], 3, G.SEED, solver="bogus")


def test_header_symbols_and_option_are_bound():
    from radar_ml_amd import _lib
    txt = open(os.path.join(ROOT, "include", "radarml.h")).read()
    for name in ("rml_smo_solve", "rml_smo_score"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, txt)
    m = re.search(r"#define\s+RML_OPT_SMO_LDS_ROWS\s+(\d+)", txt)
    assert m and int(m.group(1)) == _lib.option_id("smo_lds_rows")
    assert int(re.search(r"#define\s+RML_SMO_LDS_ROWS_MAX\s+(\d+)", txt).group(1)) == _lib.SMO_LDS_ROWS_MAX
    # the records Python fills are the header's structs: 64 and 16 bytes without padding
    import radar_ml_amd.train as T
    assert T.SMO_PROBLEM.itemsize == 64 and T.SMO_FIT.itemsize == 16
