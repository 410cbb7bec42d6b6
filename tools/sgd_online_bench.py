#!/usr/bin/env python3
"""The augmented online-learning loop of train.py:418-438 at the size of the reference's own log (train-results/train_sgd.log: 909
training and 114 test samples at the Walabot projection shapes, D = 10 010, 4 augment epochs of batch 32: 116 partial_fit + predict
pairs in 63 s), on synthetic planes.

    python tools/sgd_online_bench.py [--sklearn] [--epochs 4] [--train 909] [--test 114] [--online-steps 1000] [--out FILE]

Reports, in seconds of wall clock, each ended by a device synchronise:
  online_loop_s    the augment epochs of ``sgd_fit`` (augmentation, features, one rml_sgd_online call per epoch); the grid search in
                   front of them is replaced by one fixed candidate and not counted
  chain_s          the device part of those epochs alone (the ``partial_fit_sgd_steps`` calls)
  python_loop_s    the same step lists through a Python loop of ``partial_fit_sgd`` + ``from_sklearn(est).predict`` (what the library
                   offered before rml_sgd_online), on the same rows, in the same process
  sklearn_loop_s   with --sklearn: scikit-learn's own partial_fit + predict on the same lists
  online_learn_s   the --online_learn chain: ``--online-steps`` identical partial fits of the balanced training set in one call
and checks that the first two leave the same estimator, bit for bit.  Prints one JSON line."""
import argparse
import copy
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((22, 176), (31, 176), (22, 31))                           # xz, yz, xy of the 22 x 31 x 176 arena


def planes(n, seed, weights=(0.45, 0.35, 0.20)):
    rng = np.random.RandomState(seed)
    y = rng.choice(len(weights), size=n, p=weights)
    x = []
    for c in y:
        t = []
        for h, w in SHAPES:
            p = 0.3 * rng.rand(h, w)
            p[(3 * c) % h:(3 * c) % h + 4, :] += 0.4
            p[rng.rand(h, w) < 0.6] = 0.0
            p[0, 0] = 1.0
            t.append(p.astype(np.float32))
        x.append(tuple(t))
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--train", type=int, default=909)
    ap.add_argument("--test", type=int, default=114)
    ap.add_argument("--online-steps", type=int, default=1000)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from sklearn.linear_model import SGDClassifier
    import radar_ml_amd as rml
    import radar_ml_amd.train as T
    warnings.simplefilter("ignore")
    (x, y), (xt, yt) = planes(args.train, 1), planes(args.test, 2)
    calls, marks, start = [], {}, {}
    real = T._sgd_online

    def hook(X, plan, device=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = real(X, plan, device)
        torch.cuda.synchronize()
        calls.append((X, plan, time.perf_counter() - t0))
        return out

    def search(X, yb, cv, seed, device=None):
        est = T.fit_sgd(SGDClassifier(loss="log_loss", alpha=1e-5, penalty="l2", random_state=seed, max_iter=20), X, yb)
        start["est"] = copy.deepcopy(est)
        torch.cuda.synchronize()
        marks["search_done"] = time.perf_counter()
        return est
    T._sgd_online, T.find_best_sgd_svm_estimator = hook, search
    np.random.seed(1)
    T.sgd_fit((x[:64], y[:64]), (xt, yt), (True, True, True), False, None, epochs=1)     # warm-up: kernels loaded, workspace grown
    calls.clear()
    np.random.seed(1)
    clf = T.sgd_fit((x, y), (xt, yt), (True, True, True), False, None, epochs=args.epochs)
    torch.cuda.synchronize()
    res = {"train": args.train, "test": args.test, "D": int(calls[0][0].shape[1]), "epochs": args.epochs,
           "steps": int(sum(len(p["steps"]) for _, p, _ in calls)), "rows_per_step": float(np.mean(np.concatenate([p["steps"]["n"] for _, p, _ in calls]))),
           "online_loop_s": time.perf_counter() - marks["search_done"], "chain_s": sum(t for _, _, t in calls), "reference_log_s": 63.0}
    T._sgd_online = real
    classes = clf.classes_
    host = [(X.cpu().numpy(), plan) for X, plan, _ in calls]

    def loop(est, fit, predict):
        accs = []
        for Xh, plan in host:
            for st in plan["steps"]:
                sl = slice(int(st["off"]), int(st["off"]) + int(st["n"]))
                rows = plan["rows"][sl]
                fit(est, Xh[rows], classes[plan["cls"][sl]])
                accs.append(float(np.mean(predict(est, Xh[plan["test_rows"]]) == classes[plan["test_y"]])))
        return est, accs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    chain, _ = loop(copy.deepcopy(start["est"]), lambda e, a, b: T.partial_fit_sgd(e, a, b, classes=classes),
                    lambda e, a: rml.from_sklearn(e).predict(a))
    torch.cuda.synchronize()
    res["python_loop_s"] = time.perf_counter() - t0
    res["same_bits"] = bool(np.array_equal(chain.coef_, clf.coef_) and np.array_equal(chain.intercept_, clf.intercept_) and chain.t_ == clf.t_)
    if args.sklearn:
        t0 = time.perf_counter()
        loop(copy.deepcopy(start["est"]), lambda e, a, b: e.partial_fit(a.astype(np.float64), b, classes=classes),
             lambda e, a: e.predict(a.astype(np.float64)))
        res["sklearn_loop_s"] = time.perf_counter() - t0
    yb, Xb = T.balance_classes(y, T._feature_rows(x, (True, True, True)))
    everything = np.arange(len(yb))
    T.partial_fit_sgd_steps(copy.deepcopy(start["est"]), Xb, yb, [everything] * 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T.partial_fit_sgd_steps(copy.deepcopy(start["est"]), Xb, yb, [everything] * args.online_steps)
    torch.cuda.synchronize()
    res["online_learn_s"], res["online_steps"], res["online_rows"] = time.perf_counter() - t0, args.online_steps, int(len(yb))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
