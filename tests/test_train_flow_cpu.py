"""The host side of train.py's main after the grid search, without a GPU: ``balance_classes`` and the batches of the augment loop of
``sgd_fit`` against fixtures recorded from the reference's own functions (tests/golden/train_flow.npz, made by
make_golden_train_flow.py), and ``calibrate_prefit`` against scikit-learn's own sigmoid calibration on the same decision values."""
import importlib.util
import os
import pickle

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_train_flow", os.path.join(HERE, "golden", "make_golden_train_flow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def T(rml):
    import radar_ml_amd.train as T
    return T


@pytest.fixture(scope="module")
def G(golden):
    return golden("train_flow.npz")


@pytest.mark.parametrize("name", ["balanced", "unbalanced", "absent"])
def test_balance_classes_is_the_references(T, G, name):
    lab, data = G["bal_%s_labels" % name], G["bal_%s_data" % name]
    yb, Xb = T.balance_classes(lab, data)
    np.testing.assert_array_equal(yb, G["bal_%s_out_labels" % name])
    np.testing.assert_array_equal(Xb, G["bal_%s_out_data" % name])
    idx = T.balance_indices(lab)
    if name == "balanced":
        assert idx is None and yb is lab and Xb is data             # returned as it is
    else:
        np.testing.assert_array_equal(data[idx], Xb)
        counts = np.unique(yb, return_counts=True)[1]
        assert len(set(counts)) == 1 and counts[0] == np.unique(lab, return_counts=True)[1].max()
    # a list of labels, as svc_fit's loop builds them
    np.testing.assert_array_equal(T.balance_classes(list(lab), data)[0], G["bal_%s_out_labels" % name])


def test_augment_steps_are_the_references_batches(T, rml, G):
    """the row lists sgd_fit hands to the device for the 40-sample set: per batch the augmented tuples whose sample lies in it, in
    the reference's order, balanced as its balance_classes balances the batch (the noise values are drawn unseeded; not compared)"""
    M = _maker()
    x, y = M.flow_set()
    np.random.seed(M.FLOW_SEED)
    gen = rml.DataGenerator(rotation_range=5.0, zoom_range=0.2, noise_sd=0.1, balance=True)
    jobs, labels = gen._draw_jobs(x, y, gen._class_weights(y))
    labels = np.array(labels)
    sample_of = np.array([j[1] for j in jobs])
    steps = T._augment_steps(sample_of, labels, len(x), M.FLOW_BATCH)
    assert len(steps) == int(G["flow_batches"]) == 3
    start = 0
    for b, rows in enumerate(steps):
        want_labels = G["flow_%d_labels" % b]
        np.testing.assert_array_equal(labels[start:start + len(want_labels)], want_labels)
        np.testing.assert_array_equal(rows, start + G["flow_%d_index" % b])
        np.testing.assert_array_equal(labels[rows], G["flow_%d_balanced" % b])
        start += len(want_labels)
    assert start == len(labels)


@pytest.mark.parametrize("kind", ["sgd3", "sgd2", "svc"])
def test_calibrate_prefit(T, rml, monkeypatch, kind):
    """a_ / b_ are the bits of scikit-learn's _sigmoid_calibration on the same decision values; the object is a CalibratedClassifierCV
    that predicts, pickles and that from_sklearn's unwrapping takes"""
    from sklearn.calibration import CalibratedClassifierCV, _sigmoid_calibration
    from sklearn.linear_model import SGDClassifier
    from sklearn.preprocessing import label_binarize
    from sklearn.svm import SVC
    import radar_ml_amd.svm as svm
    rng = np.random.RandomState(0)
    nc = 2 if kind == "sgd2" else 3
    y = np.arange(90) % nc
    X = (rng.rand(90, 12) + 0.5 * np.eye(nc)[y].repeat(12 // nc, axis=1)).astype(np.float32)
    clf = (SVC(probability=True, random_state=1) if kind == "svc" else SGDClassifier(loss="log_loss", random_state=1)).fit(X[:60].astype(np.float64), y[:60])

    class Host:                                                     # the GPU twin's decision values stand in: scikit-learn's own
        def __init__(self, est):
            self.est = est

        def decision_function(self, rows):
            return self.est.decision_function(np.asarray(rows, dtype=np.float64))
    monkeypatch.setattr(svm, "from_sklearn", Host)
    Xv, yv = X[60:], y[60:]
    cal = T.calibrate_prefit(clf, Xv, yv)
    assert type(cal) is CalibratedClassifierCV and len(cal.calibrated_classifiers_) == 1 and cal.estimator is clf
    dec = clf.decision_function(Xv.astype(np.float64)).reshape(len(yv), -1)
    Y = label_binarize(yv, classes=clf.classes_)
    cals = cal.calibrated_classifiers_[0].calibrators
    assert len(cals) == dec.shape[1]
    for c, k in zip(cals, range(dec.shape[1])):
        a, b = _sigmoid_calibration(dec[:, k], Y[:, k if nc > 2 else 0])
        assert c.a_ == a and c.b_ == b
    monkeypatch.undo()
    proba = cal.predict_proba(Xv.astype(np.float64))
    assert proba.shape == (len(yv), nc) and np.allclose(proba.sum(axis=1), 1.0)
    again = pickle.loads(pickle.dumps(cal))
    np.testing.assert_array_equal(again.predict_proba(Xv.astype(np.float64)), proba)
    est, a, b = svm.unwrap_calibrated(again.calibrated_classifiers_[0])
    assert type(est) is type(clf) and list(a) == [c.a_ for c in cals] and list(b) == [c.b_ for c in cals]
    with pytest.raises(ValueError, match="inconsistent numbers of samples"):
        monkeypatch.setattr(svm, "from_sklearn", Host)
        T.calibrate_prefit(clf, Xv, yv[:-1])
