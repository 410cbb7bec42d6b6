"""The device SVC fit without a GPU: the two host functions of the library (libsvm's shuffle and its sigmoid fit) against
scikit-learn bit for bit, and ``fit_svc`` / ``GridSearchSVC(refit_solver="device")`` with the device hook (``train._smo``) replaced by
its NumPy twin (tests/smo_common.py), against ``SVC(kernel='precomputed')`` run live on the same symmetric matrix: equality."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
import smo_common as S  # noqa: E402
import svc_fit_common as F  # noqa: E402
sys.path.pop(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


def twin_smo(Xh, kernels, plan, device=None):
    """smo_common.twin_smo with the ``solve`` hook of train._smo: another plan on the same matrices"""
    out = S.twin_smo(Xh, kernels, plan, device)
    out["solve"] = lambda plan2: S.twin_smo(Xh, kernels, plan2, device)
    return out


@pytest.fixture
def twin(T, monkeypatch):
    monkeypatch.setattr(T, "_gram", G.numpy_gram)
    monkeypatch.setattr(T, "_smo", twin_smo)
    return T


def newrand_shuffle(seed, l):
    from sklearn.svm import _newrand
    _newrand.set_seed_wrap(seed)
    perm = list(range(l))
    for i in range(l):
        j = i + _newrand.bounded_rand_int_wrap(l - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm, dtype=np.int32)


@pytest.mark.parametrize("seed", [0, 1, 1234, 2 ** 31 - 2])
def test_shuffle_is_libsvms(T, seed):
    for l in (1, 2, 3, 5, 118, 4860):
        perm = T.libsvm_shuffle(seed, l)
        assert perm.dtype == np.int32 and np.array_equal(perm, newrand_shuffle(seed, l)), (seed, l)
    assert T.libsvm_shuffle(seed, 0).shape == (0,)


@pytest.mark.parametrize("k", range(len(F.REAL_KERNELS)))
def test_platt_fit_is_libsvms_on_real_xy_pairs(T, k):
    """probA_ / probB_ of SVC(probability=True) on the three class pairs of one kernel, from decision values built with
    scikit-learn alone: its generator for the shuffle, its SVC for the five sub-models of each pair"""
    from sklearn.svm import SVC
    from sklearn.utils import check_random_state
    from sklearn.utils.class_weight import compute_class_weight
    X, y = G.real_xy()
    key, C = F.REAL_KERNELS[k]
    K = F.symmetric(G.numpy_gram(X, [key])[0])
    m = F.svc("precomputed", C).fit(K, y)
    seed = check_random_state(F.SEED).randint(np.iinfo("i").max)
    w = compute_class_weight("balanced", classes=np.unique(y), y=y)
    for p, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        rows = np.concatenate([np.nonzero(y == a)[0], np.nonzero(y == b)[0]])
        yy = np.where(y[rows] == a, 1, -1)
        l = len(rows)
        perm = newrand_shuffle(seed, l)
        dec = np.zeros(l)
        for f in range(5):
            b0, e0 = f * l // 5, (f + 1) * l // 5
            tr, te = np.concatenate([perm[:b0], perm[e0:]]), perm[b0:e0]
            sub = SVC(kernel="precomputed", C=1.0, class_weight={1: C * w[a], -1: C * w[b]}).fit(K[np.ix_(rows[tr], rows[tr])], yy[tr])
            dec[te] = sub.decision_function(K[np.ix_(rows[te], rows[tr])])
        A, B, info = T.platt_fit(dec, yy.astype(np.float64))
        assert (A, B, info) == (m.probA_[p], m.probB_[p], 0), (key, (a, b), A, m.probA_[p], B, m.probB_[p])
    if key == ("rbf", 1.0):
        assert m.probA_.min() < -15                     # the steep end


def test_platt_fit_arguments(T):
    A, B, info = T.platt_fit(np.zeros(0), np.zeros(0))                  # no rows: libsvm's starting point
    assert (A, B, info) == (0.0, 0.0, 0)
    with pytest.raises(ValueError):
        T.platt_fit(np.zeros(3), np.zeros(2))
    lib = T._lib.load()
    assert lib.rml_platt_fit(None, None, 3, None, None, None) < 0 and lib.rml_last_error()
    assert lib.rml_libsvm_shuffle(1, -1, None) < 0


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_fit_svc_equals_sklearn(twin, name):
    from sklearn.exceptions import ConvergenceWarning
    case = F.cases()[name]
    X, y, key, C, extra = case
    K = F.symmetric(G.numpy_gram(X, [key])[0])
    ours, ref, w = F.check_case(twin.fit_svc, name, case, K)
    if name == "max-iter-5":
        assert ours.fit_status_ == 1 and len(w) == 1 and w[0].category is ConvergenceWarning
    else:
        assert ours.fit_status_ == 0 and not w
    if name == "no-probability":
        assert ours.probA_.shape == (0,)
    elif name == "xy-two-class":
        assert ours.dual_coef_ is not ours._dual_coef_ and np.array_equal(ours.dual_coef_, -ours._dual_coef_)
        assert np.array_equal(ours.predict_proba(X), ours.predict_proba(X)) and ours.probA_.shape == (1,)
    if name.startswith("xy-rbf"):                       # usable as scikit-learn's own: the kernel on the rows is the matrix to a few ulps
        assert np.abs(ours.decision_function(X) - ref.decision_function(K)).max() <= 1e-9
        assert np.abs(ours.predict_proba(X) - ref.predict_proba(K)).max() <= 1e-9


def test_plan_is_libsvms_cross_validation(twin):
    """the plan of the (1, 2, 37) set: three full duals first, then per pair the folds libsvm solves -- pair (0, 1) has three rows:
    two empty folds, solved on all three rows and scored by nothing"""
    X, y = F.tiny((1, 2, 37))
    yi = y.astype(np.int32)
    plan, meta = twin._fit_plan(yi, 3, [1.0, 2.0, 4.0], 77, True, True, -1, 1e-3)
    pr = plan["problems"]
    assert plan["n_classes"] == 2 and list(pr["l"][:3]) == [3, 38, 39] and list(pr["n_pos"][:3]) == [1, 1, 2]
    assert list(pr["Cp"][:3]) == [1.0, 1.0, 2.0] and list(pr["Cn"][:3]) == [2.0, 4.0, 4.0]
    sub01 = [r for r in pr[3:] if r["Cp"] == 2.0 and r["Cn"] == 1.0]            # C swapped: the -1 group first
    assert [int(r["l"]) for r in sub01].count(3) == 2                           # the two empty folds of the three-row pair
    held = [h for h in meta["held"] if h[0] == 0]
    assert sum(len(te) for _, te, _ in held) + int((meta["const_dec"][0] != 0).sum()) == 3
    assert all(int(f["n_test"]) > 0 for f in plan["fits"]) and len(plan["test_y"]) == len(plan["test_rows"])
    for r in pr[3:]:
        rr = plan["rows"][int(r["rows_off"]):int(r["rows_off"]) + int(r["l"])]
        n = int(r["n_pos"])
        assert 0 < n < int(r["l"]) and len({int(v) for v in yi[rr[:n]]}) == 1 and len({int(v) for v in yi[rr[n:]]}) == 1
        assert yi[rr[0]] > yi[rr[-1]]                                           # the pair's second class (y = -1) leads


def test_random_state_none_draws_a_seed(twin):
    X, y = F.tiny((4, 36))
    np.random.seed(99)
    want = int(np.random.RandomState(99).randint(np.iinfo("i").max))
    seen = []
    real = twin.libsvm_shuffle
    twin.libsvm_shuffle = lambda seed, l: (seen.append(seed), real(seed, l))[1]
    try:
        twin.fit_svc(F.svc(("linear", None), 1.0, random_state=None), X, y)
    finally:
        twin.libsvm_shuffle = real
    assert seen == [want]


@pytest.fixture(scope="module")
def searched(T):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    calls, fetched = [], []

    def smo(Xh, kernels, plan, device=None):
        out = twin_smo(Xh, kernels, plan, device)
        calls.append((len(kernels), len(plan["problems"]), len(plan["fits"])))
        matrix, solve = out["matrix"], out["solve"]
        out["matrix"] = lambda k: (fetched.append(k), matrix(k))[1]
        out["solve"] = lambda plan2: (calls.append(("solve", len(plan2["problems"]), len(plan2["fits"]))), solve(plan2))[1]
        return out
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "_gram", G.numpy_gram)
        mp.setattr(T, "_smo", smo)
        dev = T.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4, solver="device",
                              refit_solver="device").fit(X, y)
        seen = (list(calls), list(fetched))
        # the host refit of the same winner on the same matrix (a one-point search: the refit does not depend on the other points)
        host = T.GridSearchSVC(G.base_svc(), {k: [v] for k, v in dev.best_params_.items()}, cv=StratifiedKFold(5).split(X, y),
                               solver="device").fit(X, y)
        mixed = T.GridSearchSVC(G.base_svc(), {k: [v] for k, v in host.best_params_.items()}, cv=StratifiedKFold(5).split(X, y),
                                refit_solver="device").fit(X, y)
    return X, y, dev, host, mixed, seen


def test_device_refit_search_matches_gridsearchcv(searched):
    X, y, dev, host, _, (calls, fetched) = searched
    G.check_parity(dev, G.sklearn_search(X, y), X, y)
    # the search's batch, then the refit's on the same matrices: 3 duals + 15 of the Platt folds, 15 held-out parts; no matrix fetched
    assert calls == [(6, 450, 150), ("solve", 18, 15)] and fetched == []
    assert dev.refit_time_ > 0 and host.refit_time_ > 0


def test_device_refit_equals_host_refit(searched):
    _, _, dev, host, mixed, _ = searched
    assert dev.best_params_ == host.best_params_
    F.same_fit(dev.best_estimator_, host.best_estimator_)
    # a host search refitted on the device computes its matrix again: the same estimator where the parameters are the same
    assert host.best_params_ == mixed.best_params_
    F.same_fit(mixed.best_estimator_, host.best_estimator_)
    assert type(mixed.best_estimator_.fit_status_) is int and mixed.best_estimator_.probA_.shape == (3,)


def test_refusals_come_before_device_work(T, monkeypatch):
    from sklearn.svm import SVC, NuSVC

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(T, "_gram", no_device)
    monkeypatch.setattr(T, "_smo", no_device)
    X, y = G.real_xy()
    X, y = X[:60], y[:60]
    with pytest.raises(ValueError, match="refit_solver"):
        T.GridSearchSVC(G.base_svc(), G.GRID, refit_solver="bogus").fit(X, y)
    with pytest.raises(ValueError, match="refit_solver"):
        T.find_best_svm_estimator(X, y, 3, G.SEED, refit_solver="gpu")
    for bad, exc in ((NuSVC(), NotImplementedError), (SVC(kernel="poly"), NotImplementedError), (SVC(kernel="rbf"), NotImplementedError),
                     (SVC(kernel="rbf", gamma="auto"), NotImplementedError), (SVC(kernel="rbf", gamma=-1.0), ValueError),
                     (SVC(kernel="linear", C=0.0), ValueError), (SVC(kernel="precomputed"), NotImplementedError)):
        with pytest.raises(exc):
            T.fit_svc(bad, X, y)
    with pytest.raises(ValueError, match="classes"):
        T.fit_svc(SVC(kernel="linear"), X, np.zeros(len(y)))
    with pytest.raises(ValueError, match="classes"):
        T.fit_svc(SVC(kernel="linear"), X, np.arange(len(y)) % 9)
    with pytest.raises(ValueError, match="inconsistent"):
        T.fit_svc(SVC(kernel="linear"), X, y[:-1])
    with pytest.raises(ValueError, match="float32"):
        T.fit_svc(SVC(kernel="linear"), X.astype(np.float64) + 1e-12, y)


def test_header_binding_and_public_surface(rml):
    import inspect
    from radar_ml_amd import _lib
    txt = open(os.path.join(ROOT, "include", "radarml.h")).read()
    for name in ("rml_libsvm_shuffle", "rml_platt_fit"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, txt)
    assert rml.fit_svc is rml.train.fit_svc and "fit_svc" in rml.__all__
    assert inspect.signature(rml.GridSearchSVC).parameters["refit_solver"].default == "host"
    assert inspect.signature(rml.find_best_svm_estimator).parameters["refit_solver"].default == "host"
    assert list(inspect.signature(rml.fit_svc).parameters) == ["estimator", "X", "y", "device"]
