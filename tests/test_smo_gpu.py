"""rml_smo_solve / rml_smo_score on the GPU against scikit-learn run live on the same matrices: equality, not a tolerance -- n_iter,
the support set, alpha against |dual_coef_| and rho against intercept_ bit for bit -- then GridSearchSVC(solver="device") end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
import smo_common as S  # noqa: E402
sys.path.pop(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


def run(T, probs, **kw):
    import torch
    mats, plan = S.make_plan(T, probs, **kw)
    out = T.smo_device(torch.from_numpy(mats).cuda(), plan)
    return out, S.split_alpha(plan, out["alpha"])


def check_all(probs, out, alphas, **kw):
    for i, prob in enumerate(probs):
        S.check_against_sklearn(prob, alphas[i], out["rho"][i], out["n_iter"][i], **kw)


@pytest.fixture(scope="module")
def real_run(T):
    """the twelve real XY duals in one batch, default settings (state in LDS)"""
    return run(T, S.real_problems())


def test_real_xy_pairs(real_run):
    out, alphas = real_run
    check_all(S.real_problems(), out, alphas)
    assert not out["stopped"].any()
    assert out["n_iter"].max() > 1000               # the fixture reaches shrinking passes (period min(l, 1000) = l here)


def test_without_shrinking(T):
    out, alphas = run(T, S.real_problems(), shrinking=False)
    check_all(S.real_problems(), out, alphas, shrinking=False)


def test_early_stop(T):
    out, alphas = run(T, S.real_problems(), max_iter=50)
    check_all(S.real_problems(), out, alphas, max_iter=50)
    want = [int(S.sklearn_fit(p)[0] >= 50) for p in S.real_problems()]           # stopped early where the full solve needs more
    assert list(out["stopped"]) == want and sum(want) >= 6
    assert all(it == 50 for it, w in zip(out["n_iter"], want) if w)


def test_early_stop_after_shrinking(T, rml_opt):
    """max_iter = 600 on the 469-row linear C = 10 dual: stopped after its first shrink pass (counter = l + 1 = 470), so with
    active_size < l -- alpha scattered back through the permuted active_set, rho over the active positions only"""
    prob = S.real_problems()[5]
    assert len(prob["rows"]) == 469 and S.sklearn_fit(prob)[0] > 600
    for cap in (None, 0):
        if cap is not None:
            rml_opt("smo_lds_rows", cap)
        out, alphas = run(T, [prob], max_iter=600)
        check_all([prob], out, alphas, max_iter=600)
        assert out["stopped"][0] == 1 and out["n_iter"][0] == 600


def test_global_variant_same_bits(T, rml_opt, real_run):
    """LDS cap 0: every dual on the workspace variant of the kernel"""
    rml_opt("smo_lds_rows", 0)
    out, alphas = run(T, S.real_problems())
    check_all(S.real_problems(), out, alphas)
    assert np.array_equal(out["alpha"], real_run[0]["alpha"]) and np.array_equal(out["rho"], real_run[0]["rho"])
    assert np.array_equal(out["n_iter"], real_run[0]["n_iter"])
    copies, two = S.degenerate_problems()
    for prob in (copies, two):
        o, a = run(T, [prob])
        check_all([prob], o, a)


def test_past_1000_rows(T, rml_opt):
    """2 400 rows: the shrink counter is min(l, 1000); in LDS (141 KB of state), and the linear one again on the workspace"""
    probs = S.big_problems()
    out, alphas = run(T, probs)
    check_all(probs, out, alphas)
    assert out["n_iter"].min() > 2000
    rml_opt("smo_lds_rows", 2048)
    o2, a2 = run(T, probs[:1])
    assert np.array_equal(a2[0], alphas[0]) and o2["rho"][0] == out["rho"][0] and o2["n_iter"][0] == out["n_iter"][0]


def test_degenerate_problems(T):
    copies, two = S.degenerate_problems()
    out, alphas = run(T, [copies])
    check_all([copies], out, alphas)
    assert out["n_iter"][0] == 6                    # quad_coef = 0 between copies: the TAU branch
    out, alphas = run(T, [two])
    check_all([two], out, alphas)
    assert out["n_iter"][0] == 1


def test_batch_equals_single_calls_and_repeats(T, real_run):
    probs = S.real_problems()
    out, alphas = real_run
    again, _ = run(T, probs)
    for k in ("alpha", "rho", "n_iter", "stopped"):
        assert np.array_equal(out[k], again[k]), k
    for i, prob in enumerate(probs):
        o, a = run(T, [prob])
        assert np.array_equal(a[0], alphas[i]) and o["rho"][0] == out["rho"][i] and o["n_iter"][0] == out["n_iter"][i], prob["name"]
    # the real set in mixed order and settings of its own: a problem's result does not depend on its neighbours
    mixed = list(reversed(probs))
    o, a = run(T, mixed, shrinking=False, max_iter=300)
    for i, prob in enumerate(mixed):
        o1, a1 = run(T, [prob], shrinking=False, max_iter=300)
        assert np.array_equal(a1[0], a[i]) and o1["n_iter"][0] == o["n_iter"][i] and o1["stopped"][0] == o["stopped"][i]


def test_batch_of_every_problem_on_both_variants(T, rml_opt, real_run):
    """every problem of this file in ONE call (matrices of 2, 12, 491 and 2 400 rows in one zero-padded stack: problems address
    rows by index) equals the one-problem calls bit for bit and a second run -- with everything in LDS (the launch's dynamic LDS
    sized by the 2 400-row duals and shared with the two-row one), and with the cap between the sizes (2048: the 2 400-row duals
    on the workspace, the others in LDS; 200: only the 118-, 12- and 2-row duals in LDS), so that one call launches both variants"""
    import torch
    everything = S.real_problems() + S.big_problems() + S.degenerate_problems()
    mats, plan = S.make_plan(T, everything)
    assert mats.shape == (8, 2400, 2400) and sorted(set(plan["problems"]["l"])) == [2, 12, 118, 395, 469, 2400]
    Kd = torch.from_numpy(mats).cuda()
    singles = []
    for i, prob in enumerate(S.real_problems()):
        singles.append((real_run[0]["n_iter"][i], real_run[1][i], real_run[0]["rho"][i]))       # = its one-problem call: the test above
    for prob in S.big_problems() + S.degenerate_problems():
        o, a = run(T, [prob])
        singles.append((o["n_iter"][0], a[0], o["rho"][0]))
    for cap in (None, 2048, 200):
        if cap is not None:
            rml_opt("smo_lds_rows", cap)
        out = T.smo_device(Kd, plan)
        alphas = S.split_alpha(plan, out["alpha"])
        for k, (it, a, rho) in enumerate(singles):
            assert out["n_iter"][k] == it and np.array_equal(alphas[k], a) and out["rho"][k] == rho, (cap, everything[k]["name"])
        assert not out["stopped"].any()
        again = T.smo_device(Kd, plan)
        for key in ("alpha", "rho", "n_iter", "stopped"):
            assert np.array_equal(out[key], again[key]), (cap, key)


def test_bad_held_out_row_is_reported_not_read(T):
    import torch
    prob = S.degenerate_problems()[0]
    mats, plan = S.make_plan(T, [prob])
    plan["fits"] = np.array([(0, 2, 0)], dtype=T.SMO_FIT)
    plan["test_rows"] = np.array([0, 12], np.int32)         # one past the matrix
    plan["test_y"] = np.zeros(2, np.int32)
    with pytest.raises(Exception, match="row outside"):
        T.smo_device(torch.from_numpy(mats).cuda(), plan)
    plan["test_rows"] = np.array([0, 11], np.int32)
    out = T.smo_device(torch.from_numpy(mats).cuda(), plan)
    assert np.isfinite(out["dec"]).all() and (out["labels"] >= 0).all()


def test_bad_row_index_is_reported_not_read(T):
    import copy
    prob = copy.copy(S.degenerate_problems()[0])
    prob["rows"] = prob["rows"].copy()
    prob["rows"][3] = 12                            # one past the matrix
    with pytest.raises(Exception, match="row outside"):
        run(T, [prob])


def test_scoring_against_svc_predict(T):
    """two fits (linear C = 10, RBF gamma = 0.001 C = 100) of the first of five stratified folds of the real XY rows, on rml_gram's
    matrices: labels = SVC.predict(K[te, tr]), split score equal, decision values within the rounding of a reordered sum"""
    from sklearn.model_selection import StratifiedKFold
    from sklearn.svm import SVC
    X, y = G.real_xy()
    tr, te = next(StratifiedKFold(5).split(X, y))
    grid = [{"C": [10.0], "kernel": ["linear"]}, {"C": [100.0], "gamma": [0.001], "kernel": ["rbf"]}]
    gs = T.GridSearchSVC(G.base_svc(), grid, cv=[(tr, te)], solver="device")
    candidates, base = gs._check()
    kernels = [("linear", None), ("rbf", 0.001)]
    plan, on_device, host = gs._smo_plan(candidates, base, kernels, [(tr, te)], y)
    assert on_device == [(0, 0), (1, 0)] and host == []
    out = T._smo(X, kernels, plan)
    for f, (kind, C) in enumerate((("linear", 10.0), ("rbf", 100.0))):
        K = out["matrix"](f)
        assert np.array_equal(K, K.T)
        m = SVC(kernel="precomputed", C=C, class_weight="balanced", decision_function_shape="ovo").fit(K[np.ix_(tr, tr)], y[tr])
        ref = m.decision_function(K[np.ix_(te, tr)])
        F = plan["fits"][f]
        sl = slice(int(F["test_off"]), int(F["test_off"]) + int(F["n_test"]))
        dec = out["dec"][sl]
        # the bound and the no-near-tie pre-check from scikit-learn's model alone: per pair (a, b) the coefficients of the class-a
        # SVs are dual_coef_[b - 1], those of the class-b SVs dual_coef_[a] (libsvm's sv_coef layout)
        Kt = np.abs(K[np.ix_(te, tr[m.support_])])
        start = np.concatenate([[0], np.cumsum(m.n_support_)])
        bound = np.zeros_like(ref)
        for p, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
            sa, sb = slice(start[a], start[a + 1]), slice(start[b], start[b + 1])
            ca, cb = np.abs(m.dual_coef_[b - 1, sa]), np.abs(m.dual_coef_[a, sb])
            n_sv = int((ca > 0).sum() + (cb > 0).sum())
            bound[:, p] = 4 * n_sv * 2.0 ** -53 * (Kt[:, sa] @ ca + Kt[:, sb] @ cb)
            assert out["n_iter"][int(F["prob0"]) + p] == m.n_iter_[p]
        assert np.abs(ref).min() > 1000 * bound.max(), (np.abs(ref).min(), bound.max())      # scikit-learn alone: no near-tie in the fixture
        print("%s: max |dec - sklearn| = %.3g, smallest bound %.3g" % (kind, np.abs(dec - ref).max(), bound.min()))
        assert (np.abs(dec - ref) <= bound).all()
        assert np.array_equal(dec, ref)             # the sum runs in libsvm's order: the same bits
        pred = m.predict(K[np.ix_(te, tr)])
        assert np.array_equal(out["labels"][sl], pred)              # classes are 0, 1, 2: class index = label
        assert out["correct"][f] == (pred == y[te]).sum()
        assert out["correct"][f] / len(te) == m.score(K[np.ix_(te, tr)], y[te])


@pytest.fixture(scope="module")
def searched(rml):
    from sklearn.model_selection import StratifiedKFold
    X, y = G.real_xy()
    dev = rml.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4, solver="device").fit(X, y)
    host = rml.GridSearchSVC(G.base_svc(), G.GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=4, solver="host").fit(X, y)
    return X, y, dev, host


def test_device_search_matches_gridsearchcv(searched):
    X, y, dev, _ = searched
    G.check_parity(dev, G.sklearn_search(X, y), X, y)      # includes: best_estimator_ pickles without the package


def test_device_search_split_scores_equal_host(searched):
    _, _, dev, host = searched
    for k in range(5):
        key = "split%d_test_score" % k
        assert np.array_equal(dev.cv_results_[key], host.cv_results_[key]), key
    assert dev.best_params_ == host.best_params_
    assert np.array_equal(dev.best_estimator_.dual_coef_, host.best_estimator_.dual_coef_)


def test_off_grid_rows_at_reference_feature_length(rml):
    """the N = 300, D = 10 010 off-grid set of tests/test_grid_search_gpu.py with solver="device": the same assertions"""
    rng = np.random.default_rng(20)
    N, D = 300, 10010
    y = np.arange(N) % 3
    centers = 0.5 + 0.03 * rng.standard_normal((3, D))
    X = np.clip(centers[y] + 0.25 * rng.standard_normal((N, D)), 0.0, 1.0).astype(np.float32)
    grid = [{"C": [0.1, 10], "kernel": ["linear"]}, {"C": [1, 100], "gamma": [1e-4, 1e-3], "kernel": ["rbf"]}]
    ours = rml.GridSearchSVC(G.base_svc(), grid, cv=5, n_jobs=4, solver="device").fit(X, y)
    ref = G.sklearn_search(X, y, grid)
    assert ours.best_params_ == ref.best_params_
    for k in range(5):
        key = "split%d_test_score" % k
        assert np.array_equal(ours.cv_results_[key], ref.cv_results_[key]), key
    assert np.array_equal(ours.best_estimator_.predict(X), ref.best_estimator_.predict(X))
