"""``fit_svc`` and ``GridSearchSVC(refit_solver="device")`` on the GPU against scikit-learn run live on rml_gram's own matrices:
equality of the fitted estimators (tests/svc_fit_common.py), on both variants of the solver kernel and run to run."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
import svc_fit_common as F  # noqa: E402
sys.path.pop(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


@pytest.fixture(scope="module")
def matrices(T):
    """rml_gram's matrix of every case, fetched once per (rows, kernel)"""
    cache = {}

    def get(name):
        X, _, key, _, _ = F.cases()[name]
        k = (id(X), key)
        if k not in cache:
            cache[k] = T._gram(X, [key])[0]
            assert np.array_equal(cache[k], cache[k].T)
        return cache[k]
    return get


@pytest.fixture(scope="module")
def first_run(rml, matrices):
    """the first real XY case, fitted once with the default settings (state in LDS)"""
    name = F.CASE_NAMES[0]
    return F.check_case(rml.fit_svc, name, F.cases()[name], matrices(name))[0]


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_fit_svc_equals_sklearn(rml, matrices, name):
    ours, _, w = F.check_case(rml.fit_svc, name, F.cases()[name], matrices(name))
    assert ours.fit_status_ == int(name == "max-iter-5") and len(w) == int(name == "max-iter-5")


def test_workspace_variant_same_bits(rml, rml_opt, matrices, first_run):
    """LDS cap 0: every dual of the fit on the workspace variant of the solver kernel"""
    rml_opt("smo_lds_rows", 0)
    name = F.CASE_NAMES[0]
    ours = F.check_case(rml.fit_svc, name, F.cases()[name], matrices(name))[0]
    F.same_fit(ours, first_run)


def test_second_run_same_bits(rml, matrices, first_run):
    name = F.CASE_NAMES[0]
    X, y, key, C, extra = F.cases()[name]
    F.same_fit(rml.fit_svc(F.svc(key, C, **extra), X, y), first_run)


def test_off_grid_rows_at_reference_feature_length(rml, T):
    """the N = 300, D = 10 010 off-grid set of tests/test_smo_gpu.py"""
    rng = np.random.default_rng(20)
    N, D = 300, 10010
    y = np.arange(N) % 3
    centers = 0.5 + 0.03 * rng.standard_normal((3, D))
    X = np.clip(centers[y] + 0.25 * rng.standard_normal((N, D)), 0.0, 1.0).astype(np.float32)
    for key, C in ((("rbf", 1e-3), 1.0), (("linear", None), 0.1)):
        F.check_case(rml.fit_svc, "off-grid", (X, y, key, C, {}), T._gram(X, [key])[0])


@pytest.fixture(scope="module")
def searched(rml, T):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    fetched = []
    real = T._smo

    def watched(Xh, ks, plan, device=None):
        out = real(Xh, ks, plan, device)
        matrix = out["matrix"]
        out["matrix"] = lambda k: (fetched.append(k), matrix(k))[1]
        return out
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "_smo", watched)
        dev = rml.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4, solver="device",
                                refit_solver="device").fit(X, y)
        n_fetched = len(fetched)
        host = rml.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4, solver="device").fit(X, y)
    return X, y, dev, host, n_fetched, len(fetched)


def test_device_refit_search_matches_gridsearchcv(searched):
    X, y, dev, _, _, _ = searched
    G.check_parity(dev, G.sklearn_search(X, y), X, y)


def test_device_refit_equals_host_refit_without_a_matrix_copy(searched):
    _, _, dev, host, n_dev, n_all = searched
    assert dev.best_params_ == host.best_params_
    F.same_fit(dev.best_estimator_, host.best_estimator_)
    assert n_dev == 0 and n_all == 1                    # the host refit fetches the winner's matrix, the device refit none
    assert dev.refit_time_ > 0 and host.refit_time_ > 0


def test_pickled_winner_does_not_name_the_package(searched):
    X, _, dev, _, _, _ = searched
    blob = pickle.dumps(dev.best_estimator_)
    assert b"radar_ml_amd" not in blob and b"radar-ml_amd" not in blob
    assert np.array_equal(pickle.loads(blob).predict_proba(X), dev.best_estimator_.predict_proba(X))
