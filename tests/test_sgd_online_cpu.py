"""rml_sgd_online's semantics without a GPU: the NumPy twin of the step chain (tests/sgd_online_common.py: one ``plain_sgd`` epoch per
step plus the intercept state machine) in scikit-learn's summation order against live ``SGDClassifier.partial_fit`` chains, and
``partial_fit_sgd_steps`` with its device hook (``train._sgd_online``) replaced by that twin: the estimator it returns, its aliasing,
its accuracies and its argument checks."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_common as S  # noqa: E402
import sgd_online_common as O  # noqa: E402
sys.path.pop(0)


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


@pytest.fixture
def twin(T, monkeypatch):
    calls = []
    monkeypatch.setattr(T, "_sgd_online", O.twin_online_hook("sequential", calls))
    return calls


PAIRS = [(nc, case) for nc in (3, 2) for case in O.CASES]


@pytest.mark.parametrize("nc,case", PAIRS)
def test_twin_chain_is_sklearn(T, twin, nc, case):
    """after every prefix of the steps: t_ equal, intercepts equal, weights equal without averaging and within 1e-14 max|coef| with
    it (the twin adds to the averaged weights in its own formula order); intercept_ is _average_intercept exactly when scikit-learn's
    is; the accuracies are accuracy_score of scikit-learn's estimator after each step"""
    from sklearn.metrics import accuracy_score
    X, y = O.rows(nc)
    steps = O.step_lists(nc)
    te, te_y = O.held_out(nc)
    want = O.sklearn_chain(nc, case)
    averaged = bool(O.CASES[case].get("average", False))
    for j in range(1, len(steps) + 1):
        est, acc = T.partial_fit_sgd_steps(O.new_estimator(case), X, y, steps[:j], classes=np.unique(y), test=(te, te_y))
        ref = want[j - 1]
        got, exp = O.state_of(est), O.state_of(ref)
        assert type(est) is type(ref) and est.t_ == ref.t_ and est.n_iter_ == 1
        assert got["flag"] == exp["flag"], "step %d: intercept_ is _average_intercept" % j
        scale = float(np.abs(ref.coef_).max()) or 1.0
        for p, q in zip(got["probs"], exp["probs"]):
            assert p["intercept"] == q["intercept"] and p["avg_intercept"] == q["avg_intercept"], "step %d" % j
            if averaged:
                assert np.abs(p["coef"] - q["coef"]).max() <= 1e-14 * scale and np.abs(p["avg_coef"] - q["avg_coef"]).max() <= 1e-14 * scale
            else:
                assert np.array_equal(p["coef"], q["coef"])
        assert np.array_equal(est.intercept_, ref.intercept_)
        assert np.abs(est.coef_ - ref.coef_).max() <= (1e-14 * scale if averaged else 0.0)
        assert len(acc) == j
        for s in range(j):
            assert acc[s] == accuracy_score(te_y, want[s].predict(X[te].astype(np.float64)))
    assert len(twin) == len(steps)                                  # one device call per chain


def test_average_switches_on_inside_a_step():
    """the fixture: t_ after the steps is 2, 4, 11, 44, 51, 91, so average=10 starts in step 2 and average=45 in step 4"""
    ts = [e.t_ for e in O.sklearn_chain(3, "l2")]
    assert ts == [2.0, 4.0, 11.0, 44.0, 51.0, 91.0]
    for case, first in (("l2_avg10", 2), ("en_avg45", 4)):
        flags = [O.state_of(e)["flag"] for e in O.sklearn_chain(3, case)]
        assert flags == [s >= first for s in range(6)]


@pytest.mark.parametrize("nc,case", [(3, "en_avg45"), (2, "l2_avg10"), (3, "l1")])
def test_split_chain_and_score_every(T, twin, nc, case):
    """two calls (steps 0..j, then j..) leave the estimator of the one call; score_every=2 scores the steps 1, 3, 5"""
    X, y = O.rows(nc)
    steps = O.step_lists(nc)
    te = O.held_out(nc)
    one, acc = T.partial_fit_sgd_steps(O.new_estimator(case), X, y, steps, classes=np.unique(y), test=te, score_every=2)
    assert np.isnan(acc[[0, 2, 4]]).all() and not np.isnan(acc[[1, 3, 5]]).any()
    assert [int(c) for c in twin[-1]["steps"]["score"]] == [0, 1, 0, 1, 0, 1]
    for j in range(1, len(steps)):
        est = O.new_estimator(case)
        T.partial_fit_sgd_steps(est, X, y, steps[:j], classes=np.unique(y))
        T.partial_fit_sgd_steps(est, X, y, steps[j:])
        assert O.same_bits(O.state_of(est), O.state_of(one)), j
    again = pickle.loads(pickle.dumps(one))
    assert O.same_bits(O.state_of(again), O.state_of(one))


def test_random_state_instance_draws_per_step(T, twin):
    """a RandomState instance gives every call new seeds, as scikit-learn draws them; an integer repeats them"""
    X, y = O.rows(3)
    steps = O.step_lists(3)
    est = O.new_estimator("l2", random_state=np.random.RandomState(3))
    ref = O.new_estimator("l2", random_state=np.random.RandomState(3))
    T.partial_fit_sgd_steps(est, X, y, steps, classes=np.unique(y))
    for rr in steps:
        ref.partial_fit(X[rr].astype(np.float64), y[rr], classes=np.unique(y))
    assert np.array_equal(est.coef_, ref.coef_) and np.array_equal(est.intercept_, ref.intercept_)
    seeds = twin[-1]["steps"]["seed"][:, :3]
    assert len({tuple(s) for s in seeds}) == len(steps)
    T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, steps, classes=np.unique(y))
    assert len({tuple(s) for s in twin[-1]["steps"]["seed"][:, :3]}) == 1


def test_identical_steps_share_their_rows(T, twin):
    X, y = O.rows(3)
    everything = np.arange(O.N_ROWS)
    T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, [everything] * 4, classes=np.unique(y))
    plan = twin[-1]
    assert len(plan["rows"]) == O.N_ROWS and list(plan["steps"]["off"]) == [0] * 4


def test_checks(T, twin):
    from sklearn.linear_model import SGDClassifier
    from sklearn.svm import SVC
    X, y = O.rows(3)
    steps = O.step_lists(3)
    with pytest.raises(NotImplementedError):
        T.partial_fit_sgd_steps(SVC(), X, y, steps, classes=np.unique(y))
    with pytest.raises(NotImplementedError, match="loss"):
        T.partial_fit_sgd_steps(SGDClassifier(loss="hinge"), X, y, steps, classes=np.unique(y))
    with pytest.raises(ValueError, match="classes must be passed"):
        T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, steps)
    with pytest.raises(ValueError, match="balanced"):
        T.partial_fit_sgd_steps(SGDClassifier(loss="log_loss", class_weight="balanced"), X, y, steps, classes=np.unique(y))
    with pytest.raises(ValueError, match="no rows"):
        T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, [np.zeros(0, int)], classes=np.unique(y))
    with pytest.raises(IndexError):
        T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, [np.array([len(y)])], classes=np.unique(y))
    with pytest.raises(ValueError, match="outside classes_"):
        T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, steps, classes=[0, 1])
    with pytest.raises(NotImplementedError, match="8192|8 192|at most"):
        T.partial_fit_sgd_steps(O.new_estimator("l2"), np.zeros((8193, 4), np.float32), np.arange(8193) % 3, [np.arange(8193)], classes=[0, 1, 2])
    est = O.new_estimator("l2")
    T.partial_fit_sgd_steps(est, X, y, steps[:1], classes=np.unique(y))
    with pytest.raises(ValueError, match="not the same as on last call"):
        T.partial_fit_sgd_steps(est, X, y, steps[:1], classes=[0, 1])
    with pytest.raises(ValueError, match="Number of features"):
        T.partial_fit_sgd_steps(est, X[:, :5], y, steps[:1])
    assert twin and all(len(p["steps"]) == 1 for p in twin)         # nothing reached the device before its check failed
    est, acc = T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, [], classes=np.unique(y))
    assert len(acc) == 0


def test_overflow_raises_sklearns_error(T, monkeypatch):
    X, y = O.rows(3)

    def failing(Xr, plan, device=None):
        out = O.twin_online_device(Xr, plan)
        out["status"] = np.array([1, 2, 1], np.int32)
        return out
    monkeypatch.setattr(T, "_sgd_online", failing)
    with pytest.raises(ValueError, match="Floating-point under-/overflow occurred at epoch #1"):
        T.partial_fit_sgd_steps(O.new_estimator("l2"), X, y, O.step_lists(3), classes=np.unique(y))
