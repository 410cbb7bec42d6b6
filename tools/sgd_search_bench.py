"""SGDClassifier grid search on the GPU (GridSearchSGD, rml_sgd_solve / rml_sgd_score): one JSON line.

    python tools/sgd_search_bench.py [--rows 1458] [--sklearn] [--sklearn-jobs 16]

One seeded synthetic training set of 1 458 x 10 010 rows on the code grid (float32(c / 255), three overlapping classes: the
reference's balanced training set at its feature length) and the reference's search (train.py:350-381: 35 candidates, 5 stratified
folds, three classes: 525 problems in one batch).  Reported, wall time, host-synchronised, after one warm-up search:
  solve_s        the batched rml_sgd_solve call            score_s   the batched rml_sgd_score call
  refit_s        the refit of the winner on all rows (one more solve on the resident rows, and the estimator built from it)
  total_s        one end-to-end GridSearchSGD.fit (upload, plan, solve, score, refit)
  problems, epochs, epochs_max, steps    the batch: binary problems, their epochs in total and of the longest, SGD steps in total
  us_per_step_longest   solve_s over the steps of the longest problem (an upper bound on the time of one step)
--sklearn also runs GridSearchCV(SGDClassifier) at n_jobs = --sklearn-jobs on the same rows and reports sklearn_s and whether
best_params_ and the mean test scores agree.  No figure here is a pass / fail gate.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 10010
SEED = 1234


def synth(N, seed):
    """three balanced, overlapping classes of sparse radar-like rows: a shared blob pattern, a weak per-class one, per-row noise"""
    rng = np.random.default_rng(seed)
    y = np.arange(N) % 3
    common = np.zeros(D)
    common[rng.choice(D, 600, replace=False)] = rng.uniform(60, 255, 600)
    tmpl = np.tile(common, (3, 1))
    for c in range(3):
        idx = rng.choice(D, 150, replace=False)
        tmpl[c, idx] += rng.uniform(5, 20, 150)
    X = tmpl[y] * rng.uniform(0.5, 1.0, (N, 1)) + rng.normal(0, 40, (N, D)) * (rng.random((N, D)) < 0.1)
    return (np.rint(np.clip(X, 0, 255)).astype(np.float32) / np.float32(255.0)), y


def grid():
    small_alphas = [10.0e-08, 10.0e-09, 10.0e-10]
    alphas = [10.0e-04, 10.0e-05, 10.0e-06, 10.0e-07]
    l1_ratios = [0.075, 0.15, 0.30]
    return [{'alpha': alphas, 'penalty': ['l1', 'l2'], 'average': [False]},
            {'alpha': alphas, 'penalty': ['elasticnet'], 'average': [False], 'l1_ratio': l1_ratios},
            {'alpha': small_alphas, 'penalty': ['l1', 'l2'], 'average': [True]},
            {'alpha': small_alphas, 'penalty': ['elasticnet'], 'average': [True], 'l1_ratio': l1_ratios}]


def progress(msg):
    print("[sgd_search_bench %s] %s" % (time.strftime("%H:%M:%S"), msg), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1458)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-jobs", type=int, default=16)
    args = ap.parse_args()
    import torch
    from sklearn.linear_model import SGDClassifier
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    import radar_ml_amd.train as T
    X, y = synth(args.rows, SEED)
    max_iter = int(max(np.ceil(10**6 / len(X)), 1000))
    base = lambda: SGDClassifier(loss="log_loss", max_iter=max_iter, random_state=SEED)
    res = {"tool": "sgd_search_bench", "rows": int(args.rows), "D": D, "candidates": 35, "folds": 5, "max_iter": max_iter,
           "device": torch.cuda.get_device_name(0)}
    seen = {}
    inner = T._sgd

    def spy(Xr, plan, device=None):             # the batch's size, from the plan and the result the search itself gets
        out = inner(Xr, plan, device)
        seen.update(problems=int(len(plan["problems"])), epochs=int(out["n_iter"].sum()), epochs_max=int(out["n_iter"].max()),
                    steps=int((out["n_iter"][plan["problems"]["out"]].astype(np.int64) * plan["problems"]["n"]).sum()),
                    steps_longest=int((out["n_iter"][plan["problems"]["out"]].astype(np.int64) * plan["problems"]["n"]).max()))
        return out
    T._sgd = spy
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for rep in ("warm-up", "timed"):
            progress("GridSearchSGD, %s" % rep)
            t0 = time.perf_counter()
            gs = T.GridSearchSGD(base(), grid(), cv=StratifiedKFold(n_splits=5)).fit(X, y)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
    T._sgd = inner
    res.update(solve_s=round(gs.solve_time_, 4), score_s=round(gs.score_time_, 4), refit_s=round(gs.refit_time_, 4), total_s=round(total, 4),
               best_params=gs.best_params_, best_score=round(gs.best_score_, 6), refit_n_iter=int(gs.best_estimator_.n_iter_), **seen)
    res["us_per_step_longest"] = round(1e6 * gs.solve_time_ / max(seen["steps_longest"], 1), 3)
    if args.sklearn:
        progress("GridSearchCV(SGDClassifier), n_jobs=%d" % args.sklearn_jobs)
        import threading
        done = threading.Event()

        def heartbeat():                        # GridSearchCV is silent for minutes; a runner may take silence for a hang
            while not done.wait(60.0):
                progress("GridSearchCV still running")
        threading.Thread(target=heartbeat, daemon=True).start()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            ref = GridSearchCV(base(), grid(), cv=StratifiedKFold(n_splits=5), n_jobs=args.sklearn_jobs).fit(X.astype(np.float64), y)
            res["sklearn_s"] = round(time.perf_counter() - t0, 2)
        done.set()
        res["sklearn_jobs"] = args.sklearn_jobs
        res["sklearn_refit_s"] = round(ref.refit_time_, 2)
        res["same_best_params"] = bool(ref.best_params_ == gs.best_params_)
        res["same_mean_scores"] = bool(np.array_equal(ref.cv_results_["mean_test_score"], gs.cv_results_["mean_test_score"]))
        res["mean_score_max_diff"] = float(np.abs(ref.cv_results_["mean_test_score"] - gs.cv_results_["mean_test_score"]).max())
        res["speedup"] = round(res["sklearn_s"] / total, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
