"""train.py's main after the grid search, end to end on the GPU: ``sgd_fit``'s augment epochs and its online_learn chain against the
chain of ``partial_fit_sgd`` calls on the very row lists it handed to the device (equal in bits: see test_sgd_online_gpu.py), and
``svc_fit`` + ``calibrate_prefit`` + ``evaluate_model`` against scikit-learn on the same rows."""
import copy
import logging
import pickle
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ((6, 20), (8, 20), (6, 8))                                 # xz, yz, xy: D = 328
MASK = (True, True, True)


def make_samples(n_per_class, seed):
    """planes in [0, 1] whose maximum is exactly 1, in three classes of the given sizes"""
    rng = np.random.RandomState(seed)
    y = np.concatenate([np.full(n, c) for c, n in enumerate(n_per_class)])
    rng.shuffle(y)
    x = []
    for c in y:
        planes = []
        for h, w in SHAPES:
            p = 0.25 * rng.rand(h, w)
            p[(c * 2) % h:(c * 2) % h + 2, :] += 0.5
            p[rng.rand(h, w) < 0.5] = 0.0
            p[0, 0] = 1.0
            planes.append(p.astype(np.float32))
        x.append(tuple(planes))
    return x, y


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


@pytest.fixture(scope="module")
def data():
    return make_samples((22, 16, 10), 1), make_samples((5, 4, 3), 2), make_samples((5, 4, 3), 3)


@pytest.fixture
def recorded(T, monkeypatch):
    calls = []
    real = T._sgd_online

    def hook(X, plan, device=None):
        out = real(X, plan, device)
        calls.append((X.cpu().numpy() if hasattr(X, "cpu") else np.asarray(X), plan, out))
        return out
    monkeypatch.setattr(T, "_sgd_online", hook)
    return calls


def state_of(est):
    avg = est.average > 0
    return [np.asarray(a).copy() for a in ((est._standard_coef, est._standard_intercept, est._average_coef, est._average_intercept) if avg
                                           else (est.coef_, est.intercept_))] + [np.array(est.t_), np.array(avg and est.intercept_ is est._average_intercept)]


def replay(T, rml, est, calls):
    """the chain of partial_fit_sgd calls on the recorded row lists; returns the accuracy after every step"""
    accs = []
    for X, plan, _ in calls:
        classes = est.classes_ if hasattr(est, "classes_") else None
        for st in plan["steps"]:
            sl = slice(int(st["off"]), int(st["off"]) + int(st["n"]))
            rows = plan["rows"][sl]
            T.partial_fit_sgd(est, X[rows], classes[plan["cls"][sl]], classes=classes)
            if len(plan["test_rows"]):
                accs.append(float(np.mean(rml.from_sklearn(est).predict(X[plan["test_rows"]]) == classes[plan["test_y"]])))
    return accs


@pytest.mark.parametrize("average", [False, 40])
def test_sgd_fit_epochs(T, rml, data, recorded, monkeypatch, caplog, average):
    from sklearn.linear_model import SGDClassifier
    (x, y), (xt, yt), _ = data
    start = {}

    def search(X, yb, cv, seed, device=None):                       # the grid search has its own tests: a fixed candidate stands in
        est = T.fit_sgd(SGDClassifier(loss="log_loss", alpha=1e-4, penalty="elasticnet", average=average, random_state=seed, max_iter=30), X, yb)
        start["est"] = copy.deepcopy(est)
        return est
    monkeypatch.setattr(T, "find_best_sgd_svm_estimator", search)
    np.random.seed(5)
    with caplog.at_level(logging.DEBUG, logger=T.logger.name), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = T.sgd_fit((x, y), (xt, yt), MASK, False, None, epochs=2, folds=3, batch_size=16)
    assert type(clf) is SGDClassifier and len(recorded) == 2        # one device call per epoch
    for X, plan, _ in recorded:
        assert X.shape[1] == 328 and len(plan["steps"]) == 3 and plan["steps"]["score"].all() and len(plan["test_rows"]) == len(yt)
        for st in plan["steps"]:                                    # every batch balanced
            counts = np.bincount(plan["cls"][int(st["off"]):int(st["off"]) + int(st["n"])], minlength=3)
            assert len(set(counts)) == 1
    chain = start["est"]
    chain.classes_ = clf.classes_
    accs = replay(T, rml, chain, recorded)
    for a, b in zip(state_of(clf), state_of(chain)):
        assert np.array_equal(a, b)
    logged = [float(r.getMessage().split(": ")[1].rstrip(".")) for r in caplog.records if r.getMessage().startswith("Augmented accuracy")]
    assert logged == accs and len(accs) == 6


def test_sgd_fit_online_learn(T, rml, data, recorded, monkeypatch, tmp_path):
    from sklearn.linear_model import SGDClassifier
    (x, y), (xt, yt), _ = data
    Xh = rml.process_samples(x, proj_mask=rml.ProjMask(*MASK))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = T.fit_sgd(SGDClassifier(loss="log_loss", alpha=1e-6, average=True, random_state=T.RANDOM_SEED, max_iter=20), Xh, y)
    path = tmp_path / "svm_model.pickle"
    path.write_bytes(pickle.dumps(first))
    monkeypatch.setattr(T, "_online_learn_steps", lambda n: 5)
    clf = T.sgd_fit((x, y), (xt, yt), MASK, True, str(path), epochs=0)
    assert len(recorded) == 1
    X, plan, _ = recorded[0]
    assert len(plan["steps"]) == 5 and len(plan["rows"]) == plan["steps"]["n"][0] == 66 and not plan["steps"]["score"].any()
    chain = pickle.loads(path.read_bytes())
    replay(T, rml, chain, recorded)
    for a, b in zip(state_of(clf), state_of(chain)):
        assert np.array_equal(a, b)


def test_svc_fit_calibrate_evaluate(T, rml, data, monkeypatch, tmp_path):
    from sklearn.calibration import CalibratedClassifierCV
    from sklearn.metrics import confusion_matrix
    from sklearn.svm import SVC
    (x, y), (xt, yt), (xv, yv) = data
    seen = {}
    real = T.find_best_svm_estimator

    def search(X, yb, cv, seed, **kw):
        seen["X"], seen["y"] = X, yb
        return real(X, yb, cv, seed, **kw)
    monkeypatch.setattr(T, "find_best_svm_estimator", search)
    np.random.seed(6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = T.svc_fit((list(x), y), MASK, epochs=1, folds=3)
        assert type(clf) is SVC and len(seen["y"]) == 3 * 22 * 4    # 48 + 3 x 48 rows, every class upsampled to the largest
        mask = rml.ProjMask(*MASK)
        Xv, Xt = rml.process_samples(xv, proj_mask=mask), rml.process_samples(xt, proj_mask=mask)
        cal = T.calibrate_prefit(clf, Xv, yv)
        # the all-scikit-learn pipeline on the rows the search saw: the same SVC fitted by libsvm, calibrated by CalibratedClassifierCV
        sk = SVC(**clf.get_params()).fit(seen["X"].astype(np.float64), seen["y"])
        sk_cal = CalibratedClassifierCV(sk, cv="prefit").fit(Xv.astype(np.float64), yv)
    assert type(cal) is CalibratedClassifierCV
    proba = sk_cal.predict_proba(Xt.astype(np.float64))
    srt = np.sort(proba, axis=1)
    assert (srt[:, -1] - srt[:, -2]).min() >= 1e-3                  # the fixture: no near-ties
    want = sk_cal.predict(Xt.astype(np.float64))
    gpu = rml.from_sklearn(pickle.loads(pickle.dumps(cal)))
    assert type(gpu) is rml.GpuCalibratedClassifier
    np.testing.assert_array_equal(gpu.predict(Xt), want)
    png = tmp_path / "cm.png"
    acc, cm, report = T.evaluate_model(cal, Xt, yt, ["a", "b", "c"], str(png))
    np.testing.assert_array_equal(cm, confusion_matrix(yt, want))
    assert acc == float(np.mean(want == yt)) and "precision" in report and png.stat().st_size > 0
    acc2, cm2, _ = T.evaluate_model(gpu, Xt, yt, ["a", "b", "c"])
    assert acc2 == acc and np.array_equal(cm2, cm)
