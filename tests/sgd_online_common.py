"""Shared by test_sgd_online_cpu.py and test_sgd_online_gpu.py: a NumPy twin of rml_sgd_online (``sgd_common.plain_sgd`` run one epoch per
step from the state the last step left, plus the intercept statements of _fit_binary / _fit_multiclass restated as the state machine
of include/radarml.h), the step set, the estimator cases, and scikit-learn's own partial_fit chains run live, computed once."""
import copy
import functools
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_common as S  # noqa: E402
sys.path.pop(0)

# the estimator cases (SGDClassifier keywords); the steps below make t = 2, 4, 11, 44, 51, 91, so that average=10 switches on inside
# step 2 and average=45 inside step 4
CASES = {
    "l2": dict(penalty="l2", alpha=1e-3),
    "l1": dict(penalty="l1", alpha=1e-4),
    "en": dict(penalty="elasticnet", alpha=1e-5, l1_ratio=0.15),
    "l2_avg": dict(penalty="l2", alpha=1e-7, average=True),
    "en_avg": dict(penalty="elasticnet", alpha=1e-8, l1_ratio=0.3, average=True),
    "l2_avg10": dict(penalty="l2", alpha=1e-5, average=10),
    "en_avg45": dict(penalty="elasticnet", alpha=1e-6, l1_ratio=0.15, average=45),
}
STEP_ROWS = (1, 2, 7, 33, 7, 40)
N_ROWS, N_TEST = 60, 20
DATA_SEED = {3: 11, 2: 12}


@functools.lru_cache(maxsize=None)
def rows(n_classes, D=96):
    """60 training rows and 20 held-out rows of D features (one matrix: the held-out rows are the last 20)."""
    return S.make_rows(N_ROWS + N_TEST, D, n_classes=n_classes, seed=DATA_SEED[n_classes] + D)


@functools.lru_cache(maxsize=None)
def step_lists(n_classes, D=96):
    """Steps of 1, 2, 7, 33, 7 (with a repeated row) and 40 rows out of the 60; step 2 lacks the last class."""
    _, y = rows(n_classes, D)
    rng = np.random.RandomState(5)
    out = []
    for s, n in enumerate(STEP_ROWS):
        pool = np.arange(N_ROWS)
        if s == 2:
            pool = pool[y[:N_ROWS] != n_classes - 1]
        rr = rng.choice(pool, size=n, replace=False)
        if s == 4:
            rr[-1] = rr[0]
        out.append(rr.astype(np.int64))
    assert len(set(y[out[2]])) == n_classes - 1 and len(set(y[out[5]])) == n_classes
    return out


def held_out(n_classes, D=96):
    _, y = rows(n_classes, D)
    te = np.arange(N_ROWS, N_ROWS + N_TEST)
    return te, y[te]


def new_estimator(case, random_state=S.RANDOM_STATE):
    from sklearn.linear_model import SGDClassifier
    kw = CASES[case] if isinstance(case, str) else case
    return SGDClassifier(loss="log_loss", random_state=random_state, **kw)


def state_of(est):
    """The solver's view of an estimator: per problem the standard / averaged weights and intercepts, t_, and whether intercept_ is the
    averaged array."""
    probs = [{k: np.array(v) for k, v in p.items()} for p in S.est_problems(est)]      # copies: the chain goes on writing the arrays
    return dict(probs=probs, t=est.t_, flag=bool(est.average > 0 and est.intercept_ is est._average_intercept))


@functools.lru_cache(maxsize=None)
def sklearn_chain(n_classes, case, D=96):
    """scikit-learn's own chain of partial_fit calls on the step set: a copy of the estimator after every step."""
    X, y = rows(n_classes, D)
    X64 = X.astype(np.float64)
    est = new_estimator(case)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for rr in step_lists(n_classes, D):
            est.partial_fit(X64[rr], y[rr], classes=np.unique(y))
            out.append(copy.deepcopy(est))
    return out


def same_bits(a, b):
    """Two ``state_of`` results identical in every bit."""
    if a["t"] != b["t"] or a["flag"] != b["flag"] or len(a["probs"]) != len(b["probs"]):
        return False
    return all(np.array_equal(p[k], q[k]) for p, q in zip(a["probs"], b["probs"]) for k in ("coef", "intercept", "avg_coef", "avg_intercept"))


# ---- the twin ------------------------------------------------------------------------------------------------------------------
def twin_online_device(X32, plan, order="sequential"):
    """What ``train.sgd_online_device`` returns for ``plan`` on the host rows ``X32``, computed by the twin."""
    X64 = np.asarray(X32, dtype=np.float32).astype(np.float64)
    D = X64.shape[1]
    probs, steps, C = plan["problems"], plan["steps"], int(plan["n_classes"])
    K = len(probs)
    n_dec = 1 if C == 2 else C
    init = plan["init"]
    coef, acoef = np.array(init["coef"], dtype=np.float64), np.array(init["avg_coef"], dtype=np.float64)
    SI, AI = np.array(init["intercept"], dtype=np.float64), np.array(init["avg_intercept"], dtype=np.float64)
    average = int(probs[0]["average"])
    A = bool(plan.get("avg_flag", False)) and average > 0
    t = float(probs[0]["t0"])
    te_rows, te_y = np.asarray(plan.get("test_rows", []), dtype=np.int64), np.asarray(plan.get("test_y", []), dtype=np.int64)
    n_test = len(te_rows)
    correct = np.full(len(steps), -1, dtype=np.int32)
    dec, labels = np.zeros((n_test, n_dec)), np.zeros(n_test, np.int32)
    status, fail_step = np.ones(K, np.int32), -1
    N = X64.shape[0]
    bad = any(((plan["rows"][int(s["off"]):int(s["off"]) + int(s["n"])] < 0) | (plan["rows"][int(s["off"]):int(s["off"]) + int(s["n"])] >= N)).any()
              for s in steps) or ((te_rows < 0) | (te_rows >= N)).any()
    if bad:
        status[:] = -1
        steps = []
    for s, st in enumerate(steps):
        sl = slice(int(st["off"]), int(st["off"]) + int(st["n"]))
        rr, cls = plan["rows"][sl], plan["cls"][sl]
        res = []
        for k, p in enumerate(probs):
            pos = 1 if C == 2 else k
            res.append(S.plain_sgd(X64[rr], (cls == pos).astype(np.float64), int(p["penalty"]), float(p["alpha"]), float(p["l1_ratio"]), average,
                                   1, None, 1, bool(p["shuffle"]), int(st["seed"][k]), float(p["weight_pos"]), float(p["weight_neg"]), t,
                                   (coef[k], SI[k], acoef[k], AI[k]), order))
        failed = [k for k, r in enumerate(res) if r["status"] == 2]
        if failed:
            for k in failed:
                status[k] = 2
            fail_step = s
            break
        t += len(rr)
        now = average > 0 and average <= t - 1
        for k, r in enumerate(res):
            coef[k] = r["coef"]
            if average > 0:
                acoef[k], AI[k] = r["avg_coef"], r["avg_intercept"]
            if C > 2:
                if A:
                    AI[k] = r["intercept"]
                else:
                    SI[k] = r["intercept"]
            elif not now:
                SI[k] = r["intercept"]
        A = bool(now)
        if st["score"] and n_test:
            cf, b = (acoef, AI) if A else (coef, SI)
            for r_, row in enumerate(te_rows):
                for k in range(K):
                    dec[r_, k] = S.DOTS[order](cf[k], X64[row]) + b[k]
            labels = (dec[:, 0] > 0).astype(np.int32) if C == 2 else dec.argmax(axis=1).astype(np.int32)
            correct[s] = int((labels == te_y).sum())
    return {"coef": coef, "avg_coef": acoef, "intercept": SI, "avg_intercept": AI, "t": np.full(K, t), "status": status, "avg_flag": A,
            "fail_step": fail_step, "correct": correct, "labels": labels, "dec": dec}


def twin_online_hook(order="sequential", calls=None):
    """A replacement for ``train._sgd_online``."""
    def hook(X, plan, device=None):
        if calls is not None:
            calls.append(plan)
        return twin_online_device(X, plan, order)
    return hook


def chain(T, est, X, y, steps, step, classes):
    """``step(est, X[rows], y[rows], classes)`` for every step; returns the state after each."""
    out = []
    for rr in steps:
        step(est, X[rr], y[rr], classes)
        out.append(state_of(est))
    return out
