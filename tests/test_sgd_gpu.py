"""rml_sgd_solve / rml_sgd_score on the GPU against the NumPy twin in the kernel's own summation order (tests/sgd_common.py; the twin
in scikit-learn's order IS scikit-learn, test_sgd_cpu.py), then fit_sgd, partial_fit_sgd and GridSearchSGD end to end against
scikit-learn run live.

Tolerance: n_iter, t and status are equal; weights and intercepts, over max|coef|, are within max(8 delta, 1e-12), where delta is what
re-ordering the sum alone does to the case (the larger deviation from scikit-learn of the twin in 'kernel' and in 'tree256' order).
The device differs from its twin only by its exp / log / log1p: a perturbation of the size re-ordering causes, through the same
dynamics.  Every test prints its error / delta ratio."""
import os
import pickle
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_common as S  # noqa: E402
sys.path.pop(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


def solve(T, X, plan, **kw):
    import torch
    return T.sgd_device(torch.from_numpy(np.ascontiguousarray(X)).cuda(), plan, **kw)


def check_fit(out, ref, what, slot0=0):
    """the problems slot0 .. of ``out`` against the twin fit ``ref['kernel']``"""
    probs = ref["kernel"]["probs"]
    coefs, acoefs = out["coefs"](range(slot0, slot0 + len(probs)))
    err = max(S.check_problem(out, slot0 + k, (coefs[k], acoefs[k]), w, ref["scale"], ref["tol"], "%s problem %d" % (what, k))
              for k, w in enumerate(probs))
    print("%s: error %.3g, delta %.3g, ratio %.3g, tolerance %.3g" % (what, err, ref["delta"], err / ref["delta"] if ref["delta"] else 0.0,
                                                                  ref["tol"]))
    return err


@pytest.mark.parametrize("data,case", S.PAIRS)
def test_cases(T, data, case):
    """the case grid on 150 x 640 in three classes; D = 96 (most threads own nothing); D = 1 030 (six threads own a second element);
    60 rows; two classes at 40 x 96"""
    X, y = S.dataset(data)
    ref = S.reference(data, case)
    out = solve(T, X, S.make_plan(T, [S.class_fit(X, y, case)], len(np.unique(y))))
    assert (out["status"] == 0).all()
    check_fit(out, ref, "%s %s" % (data, case))


def test_two_rows(T):
    X, _ = S.dataset("bin")
    y = np.array([0, 1])
    for case in ("l2_1e-3", "en_1e-8_avg"):
        ref = S.make_reference(X[:2], y, S.CASES[case])
        out = solve(T, X[:2], S.make_plan(T, [S.class_fit(X[:2], y, case)], 2))
        check_fit(out, ref, "two rows %s" % case)


def test_row_subset_wide_ld_and_empty_class(T):
    """a row list that is a strict subset of a matrix with ld > D (the padding is NaN: never read), and a class without a positive
    row in the list"""
    import torch
    X, y = S.dataset("main")
    big = torch.full((len(y) + 7, X.shape[1] + 5), float("nan"), dtype=torch.float32, device="cuda")
    big[:len(y), :X.shape[1]] = torch.from_numpy(X).cuda()
    Xd = big[:, :X.shape[1]]
    rows = np.nonzero(y != 2)[0][::-1].copy()[3:]                   # classes 0 and 1 only, descending, not all of them
    ylists = [(y[rows] == c).astype(np.int32) for c in range(3)]
    assert ylists[2].sum() == 0
    for case in ("l1_1e-4", "l2_1e-7_avg"):
        kw = S.CASES[case]
        plan = S.make_plan(T, [(rows, ylists, [11, 12, 13], kw)], 3)
        out = T.sgd_device(Xd, plan)
        coefs, acoefs = out["coefs"](range(3))
        for k in range(3):
            ref = S.twin_reference(X, rows, ylists[k], 11 + k, kw)
            err = S.check_problem(out, k, (coefs[k], acoefs[k]), ref["kernel"], ref["scale"], ref["tol"], "subset %s class %d" % (case, k))
            print("subset %s class %d: error %.3g, delta %.3g, tolerance %.3g" % (case, k, err, ref["delta"], ref["tol"]))


@pytest.mark.parametrize("D,n,max_iter", [(10010, 45, 3), (20480, 30, 2)])
def test_full_size_rows(T, D, n, max_iter):
    """D = 10 010: the resident capacity on every branch (elastic net and averaging together); D = 20 480: the workspace variant"""
    from radar_ml_amd import _lib
    assert (D <= _lib.SGD_RESIDENT_D_MAX) == (D == 10010)
    X, y = S.make_rows(n, D, seed=D)
    kw = dict(penalty="elasticnet", alpha=1e-8, l1_ratio=0.3, average=True, tol=None, max_iter=max_iter)
    ref = S.make_reference(X, y, kw)
    out = solve(T, X, S.make_plan(T, [S.class_fit(X, y, kw)], 3))
    assert (out["status"] == 1).all() and (out["n_iter"] == max_iter).all()
    check_fit(out, ref, "D = %d" % D)


def test_variants_batch_position_and_reruns_same_bits(T, rml_opt):
    X, y = S.dataset("main")
    fits = [S.class_fit(X, y, c) for c in S.CASES]
    plan = S.make_plan(T, fits, 3)
    a = solve(T, X, plan)
    b = solve(T, X, plan)
    # the first fit again at the end of a batch of 40 problems
    many = S.make_plan(T, (fits * 3)[:13] + [fits[0]], 3)
    assert len(many["problems"]) == 42
    c = solve(T, X, many)
    rml_opt("SGD_RESIDENT_D", 0)                                    # every problem on the workspace variant
    d = solve(T, X, plan)
    ca, cb, cd = a["coefs"](range(18)), b["coefs"](range(18)), d["coefs"](range(18))
    for other, co in ((b, cb), (d, cd)):
        for key in ("intercept", "avg_intercept", "n_iter", "t", "status"):
            assert np.array_equal(a[key], other[key]), key
        assert np.array_equal(ca[0], co[0]) and np.array_equal(ca[1], co[1])
    first, last = c["coefs"](range(3)), c["coefs"](range(39, 42))
    assert np.array_equal(first[0], last[0]) and np.array_equal(first[0], ca[0][:3])
    for key in ("intercept", "n_iter", "t"):
        assert np.array_equal(c[key][:3], c[key][39:42]) and np.array_equal(c[key][:3], a[key][:3]), key


def test_status(T):
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import SGDClassifier
    X, y = S.dataset("bin")
    fit = S.class_fit(X, y, "l2_1e-3")
    plan = S.make_plan(T, [fit, fit], 2)
    plan["rows"][len(y) + 5] = len(y)                               # the second problem names row N
    D = X.shape[1]
    plan["init"] = {"coef": np.full((2, D), 7.0), "avg_coef": np.full((2, D), 7.0), "intercept": np.full(2, 7.0),
                    "avg_intercept": np.full(2, 7.0)}
    out = solve(T, X, plan, check=False)
    assert list(out["status"]) == [0, -1]
    coefs, acoefs = out["coefs"]([1])
    assert (coefs == 7.0).all() and (acoefs == 7.0).all() and out["intercept"][1] == 7.0 and out["n_iter"][1] == 0 and out["t"][1] == 0
    good = S.reference("bin", "l2_1e-3")                            # the problem beside it is solved as ever
    want = good["kernel"]["probs"][0]
    assert out["n_iter"][0] == want["n_iter"] and out["t"][0] == want["t"]
    assert np.abs(out["coefs"]([0])[0][0] - want["coef"]).max() <= good["tol"] * good["scale"]
    with pytest.raises(T._lib.RadarMLError):
        solve(T, X, plan)
    short = S.make_plan(T, [S.class_fit(X, y, dict(penalty="l2", alpha=1e-3, max_iter=2, tol=1e-3))], 2)
    assert list(solve(T, X, short)["status"]) == [1]
    with pytest.warns(ConvergenceWarning, match="Maximum number of iteration reached"):
        T.fit_sgd(SGDClassifier(loss="log_loss", max_iter=2, tol=1e-3, random_state=0), X, y)


@pytest.mark.parametrize("data,case", [("main", "l2_1e-3"), ("main", "en_1e-8_avg"), ("bin", "l2_1e-7_avg")])
def test_scoring(T, data, case):
    """labels and the count of correct ones equal SGDClassifier.predict on the held-out rows; decision values within the solve's
    tolerance times max|coef| max|x| D"""
    X, y = S.dataset(data)
    n_tr = 2 * len(y) // 3
    tr, te = np.arange(n_tr), np.arange(n_tr, len(y))
    ref = S.make_reference(X[tr], y[tr], S.CASES[case])
    est = ref["est"]
    classes = np.unique(y)
    plan = S.make_plan(T, [S.class_fit(X[tr], y[tr], case)], len(classes), test=[(te, np.searchsorted(classes, y[te]))])
    out = solve(T, X, plan)
    want = est.decision_function(X[te].astype(np.float64)).reshape(len(te), -1)
    srt = np.sort(want, axis=1)
    assert (np.abs(want[:, 0]) if len(classes) == 2 else srt[:, -1] - srt[:, -2]).min() >= 1e-6       # the fixture: no near-ties
    bound = ref["tol"] * ref["scale"] * float(np.abs(X).max()) * X.shape[1]
    err = float(np.abs(out["dec"] - want).max())
    print("%s %s: decision error %.3g, bound %.3g" % (data, case, err, bound))
    assert err <= bound
    pred = est.predict(X[te].astype(np.float64))
    np.testing.assert_array_equal(classes[out["labels"]], pred)
    assert out["correct"][0] == int((pred == y[te]).sum())


@pytest.mark.parametrize("data,case", [("main", "l2_1e-3"), ("main", "en_1e-8_avg"), ("bin", "l2_1e-7_avg")])
def test_fitted_estimator(T, rml, data, case):
    from sklearn.linear_model import SGDClassifier
    X, y = S.dataset(data)
    ref = S.reference(data, case)
    est = T.fit_sgd(SGDClassifier(loss="log", max_iter=1000.0, random_state=S.RANDOM_STATE, **S.CASES[case]), X, y)
    assert type(est) is SGDClassifier and est.n_iter_ == ref["est"].n_iter_ and est.t_ == ref["est"].t_
    assert S.deviation(S.est_problems(est), S.est_problems(ref["est"]), ref["scale"]) <= ref["tol"]
    X64 = X.astype(np.float64)
    labels = est.predict(X64)
    np.testing.assert_array_equal(labels, ref["est"].predict(X64))
    proba = est.predict_proba(X64)
    assert proba.shape == (len(y), len(est.classes_)) and np.allclose(proba.sum(axis=1), 1.0)
    again = pickle.loads(pickle.dumps(est))
    np.testing.assert_array_equal(again.predict(X64), labels)
    assert np.array_equal(again.coef_, est.coef_)
    gpu = rml.from_sklearn(est)
    assert type(gpu) is rml.GpuLinearClassifier
    np.testing.assert_array_equal(gpu.predict(X), labels)


@pytest.mark.parametrize("case", ["l2_1e-3", "l2_1e-7_avg"])
def test_partial_fit_twice(T, monkeypatch, case):
    """partial_fit_sgd twice against partial_fit twice: t_ equal, weights within the tolerance (delta from the same two calls with
    the twin as the device, in 'kernel' and 'tree256' order)"""
    from sklearn.linear_model import SGDClassifier
    X, y = S.dataset("main")
    kw = S.CASES[case]
    half = len(y) // 2
    new = lambda: SGDClassifier(loss="log_loss", random_state=S.RANDOM_STATE, **kw)

    def twice(step):
        est = new()
        for sl in (slice(0, half), slice(half, None)):
            step(est, X[sl], y[sl])
        return est
    want = twice(lambda e, a, b: e.partial_fit(a.astype(np.float64), b, classes=np.unique(y)))
    got = twice(lambda e, a, b: T.partial_fit_sgd(e, a, b, classes=np.unique(y)))
    scale = float(np.abs(want.coef_).max())
    delta = 0.0
    for order in ("kernel", "tree256"):
        with monkeypatch.context() as m:
            m.setattr(T, "_sgd", S.twin_hook(order))
            tw = twice(lambda e, a, b: T.partial_fit_sgd(e, a, b, classes=np.unique(y)))
        delta = max(delta, S.deviation(S.est_problems(tw), S.est_problems(want), scale))
    err = S.deviation(S.est_problems(got), S.est_problems(want), scale)
    print("partial_fit twice %s: error %.3g, delta %.3g, tolerance %.3g" % (case, err, delta, max(8 * delta, 1e-12)))
    assert got.t_ == want.t_ == 1.0 + len(y)
    assert err <= max(8 * delta, 1e-12)
    assert S.scaled_err(got.coef_, got.intercept_, want.coef_, want.intercept_) <= max(8 * delta, 1e-12)


def test_search_end_to_end(T):
    from sklearn.linear_model import SGDClassifier
    X, y = S.search_rows()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gs = T.GridSearchSGD(SGDClassifier(loss="log_loss", random_state=S.RANDOM_STATE), S.SEARCH_GRID, cv=S.SEARCH_CV).fit(X, y)
    ref = S.check_search(gs)
    np.testing.assert_array_equal(gs.predict(X.astype(np.float64)), ref.predict(X.astype(np.float64)))
    assert gs.best_estimator_.n_iter_ == ref.best_estimator_.n_iter_
