"""SVC grid search on GPU kernel matrices (GridSearchSVC, rml_gram): one JSON line.

    python tools/grid_search_bench.py [--sets 1458,7290] [--jobs 4,16] [--solver host|device] [--refit host|device] [--sklearn]

Two seeded synthetic training sets at the reference's feature length D = 10 010 (three planes of the Walabot grid):
  1458 x 10010  rows on the code grid, float32(c/255) (the reference's balanced training set, train.py:534)
  7290 x 10010  off-grid rows (its 4-epoch augmented set, train.py:496-517)
and the reference's grid (5 linear + 25 RBF points, 5 stratified folds).  Per set:
  gram_ms        rml_gram of the six distinct kernels in one call, HIP events; gram_frac = N(N+1)D FLOP / time / 78.6 TF
  d2h_ms         the six N x N float64 matrices to the host
  host_s_jJ      the search on the host (libsvm fits on the precomputed matrices) with n_jobs = J
  total_s        one end-to-end GridSearchSVC.fit (upload, Gram, copy, search, refit) at the largest n_jobs
--solver device times GridSearchSVC(solver="device") instead (the duals solved by rml_smo_solve on the resident matrices): per n_jobs
(used only by the refit-free host fall-backs, so the figures should agree) device_search_s_jJ end to end, plus of the last run
  smo_solve_ms / smo_score_ms   wall time of the batched rml_smo_solve / rml_smo_score calls, host-synchronised
  smo_problems, smo_iters, smo_iters_max   duals in the batch, their libsvm iterations in total and of the longest dual
  refit_s        the refit of the winner (probability=True), part of every search: --refit host (the default) is libsvm on the
                 host copy of the winner's matrix, --refit device the same fit as one batch of duals on the resident matrix
                 (GridSearchSVC(refit_solver="device")); refit_solver names which one the line timed
--sklearn also runs scikit-learn's GridSearchCV on the raw rows of the 1458 set, on the sub-grid stated in the output (the full grid
runs for about an hour), and reports its time and whether best_params_ agree with GridSearchSVC on the same sub-grid.

--masks [--segments 3872,5457,682] [--reps 5] times the projection-mask search instead (ProjMaskSearchSVC: the seven masks x the
reference's grid from one rml_gram_segments pass) on the first of --sets, against the loop it replaces -- the seven masks through
GridSearchSVC on column subsets, same --solver / --refit / n_jobs -- in the same process, the two alternating, --reps times each:
  mask_search_s / loop_s          medians of the end-to-end wall times (each list is in the line too)
  gram_segments_ms, compose_ms    rml_gram_segments of the rows and rml_gram_compose of the 42 matrices, HIP events, medians
  solve_ms, score_ms, refit_s     of the last mask search: the batched solve / score calls (--solver device; the sum of the host
                                  fits' times otherwise) and the refit of the winner
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_PEAK = 78.6e12
D = 10010
CS = [0.01, 0.1, 1, 10, 100]
GAMMAS = [0.001, 0.01, 0.1, 1, 10]
GRID = [{"C": CS, "kernel": ["linear"]}, {"C": CS, "gamma": GAMMAS, "kernel": ["rbf"]}]
SUB_GRID = [{"C": [1, 10], "kernel": ["linear"]}, {"C": [1, 10], "gamma": [0.001, 0.01], "kernel": ["rbf"]}]


def synth(N, on_grid, seed, D=D):
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
    X = np.clip(X, 0, 255)
    if on_grid:
        return (np.rint(X).astype(np.float32) / np.float32(255.0)), y
    return np.clip(X / 255.0 + rng.normal(0, 0.02, (N, D)), 0.0, 1.0).astype(np.float32), y


def progress(msg):
    print("[grid_search_bench %s] %s" % (time.strftime("%H:%M:%S"), msg), file=sys.stderr, flush=True)


def base_svc():
    from sklearn import svm
    return svm.SVC(probability=True, class_weight="balanced", random_state=1234, cache_size=1000, verbose=False)


def gram_timing(rml, X, kernels, reps=3):
    import torch
    from radar_ml_amd import _lib
    lib, ctx = _lib.load(), _lib.context()
    N = X.shape[0]
    kinds = np.array([_lib.GRAM_LINEAR if k == "linear" else _lib.GRAM_RBF for k, _ in kernels], dtype=np.int32)
    gammas = np.array([0.0 if g is None else g for _, g in kernels], dtype=np.float64)
    Xd = torch.from_numpy(X).cuda()
    out = torch.empty((len(kernels), N, N), dtype=torch.float64, device="cuda")
    call = lambda: _lib.check(lib.rml_gram(ctx, _lib.ptr(Xd), D, N, D, len(kernels), kinds.ctypes.data, gammas.ctypes.data,
                                           _lib.ptr(out), N, N * N, _lib.stream_ptr()), "rml_gram")
    call()                                  # warm-up (workspace growth, code load)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    host = out.cpu().numpy()
    d2h = (time.perf_counter() - t0) * 1e3
    del out, Xd
    torch.cuda.empty_cache()
    return min(ms), d2h, [host[k] for k in range(len(kernels))]


def run_set_device(rml, N, on_grid, jobs, seed, refit="host"):
    """GridSearchSVC(solver="device") end to end per n_jobs, with the batch's own figures (train._smo wrapped, not replaced)"""
    from sklearn.model_selection import StratifiedKFold
    import radar_ml_amd.train as T
    X, y = synth(N, on_grid, seed)
    res = {"rows": N, "D": D, "on_code_grid": on_grid, "solver": "device", "refit_solver": refit}
    real = T._smo
    seen = []

    def watched(Xh, ks, plan, device=None):
        out = real(Xh, ks, plan, device)
        seen.append((len(plan["problems"]), out["solve_s"], out["score_s"], int(out["n_iter"].sum()), int(out["n_iter"].max()),
                     int(plan["problems"]["l"].max())))
        return out
    T._smo = watched
    try:
        T.GridSearchSVC(base_svc(), GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=min(jobs), solver="device",
                        refit_solver=refit).fit(X, y)   # warm-up
        for j in sorted(jobs):
            del seen[:]
            t0 = time.perf_counter()
            gs = T.GridSearchSVC(base_svc(), GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=j, solver="device",
                                 refit_solver=refit).fit(X, y)
            res["device_search_s_j%d" % j] = round(time.perf_counter() - t0, 3)
            progress("%d rows: device search at n_jobs=%d: %.3f s (solve %.1f ms, score %.1f ms, refit %.3f s)"
                     % (N, j, res["device_search_s_j%d" % j], 1e3 * sum(s[1] for s in seen), 1e3 * sum(s[2] for s in seen), gs.refit_time_))
    finally:
        T._smo = real
    res.update({"smo_solve_ms": round(1e3 * sum(s[1] for s in seen), 2), "smo_score_ms": round(1e3 * sum(s[2] for s in seen), 2),
                "smo_problems": sum(s[0] for s in seen), "smo_iters": sum(s[3] for s in seen), "smo_iters_max": max(s[4] for s in seen),
                "smo_rows_max": max(s[5] for s in seen), "refit_s": round(gs.refit_time_, 3),
                "best_params": gs.best_params_, "best_score": round(gs.best_score_, 4)})
    return res, X, y


def run_set(rml, N, on_grid, jobs, seed, refit="host"):
    from sklearn.model_selection import StratifiedKFold
    import radar_ml_amd.train as T
    X, y = synth(N, on_grid, seed)
    kernels = [("linear", None)] + [("rbf", float(g)) for g in GAMMAS]
    gram_ms, d2h_ms, mats = gram_timing(rml, X, kernels)
    progress("%d rows: rml_gram %.2f ms, copy %.0f ms" % (N, gram_ms, d2h_ms))
    flop = float(N) * (N + 1) * D
    res = {"rows": N, "D": D, "on_code_grid": on_grid, "refit_solver": refit, "kernels": len(kernels), "gram_ms": round(gram_ms, 3),
           "gram_tflops": round(flop / gram_ms / 1e9, 2), "gram_frac": round(flop / (gram_ms * 1e-3) / F64_PEAK, 3),
           "d2h_ms": round(d2h_ms, 1)}
    cached = dict(zip(kernels, mats))
    real = T._gram
    best = None
    for j in sorted(jobs)[:-1]:
        T._gram = lambda Xh, ks, device=None: [cached[k] for k in ks]
        try:
            t0 = time.perf_counter()
            gs = T.GridSearchSVC(base_svc(), GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=j, refit_solver=refit).fit(X, y)
            res["host_s_j%d" % j] = round(time.perf_counter() - t0, 2)
            progress("%d rows: host search at n_jobs=%d: %.2f s" % (N, j, res["host_s_j%d" % j]))
            best = gs.best_params_
        finally:
            T._gram = real
    del mats, cached
    j = max(jobs)
    spent = [0.0]

    def timed(Xh, ks, device=None):
        t = time.perf_counter()
        try:
            return real(Xh, ks, device)
        finally:
            spent[0] += time.perf_counter() - t
    T._gram = timed
    try:
        t0 = time.perf_counter()
        gs = T.GridSearchSVC(base_svc(), GRID, cv=StratifiedKFold(5).split(X, y), n_jobs=j, refit_solver=refit).fit(X, y)
        total = time.perf_counter() - t0
    finally:
        T._gram = real
    res["host_s_j%d" % j] = round(total - spent[0], 2)
    res["device_s"] = round(spent[0], 2)
    res["total_s"] = round(total, 2)
    progress("%d rows: end to end at n_jobs=%d: %.2f s" % (N, j, total))
    res["refit_s"] = round(gs.refit_time_, 3)
    res["best_params"] = gs.best_params_
    res["best_score"] = round(gs.best_score_, 4)
    if best is not None:
        res["best_params_agree_across_jobs"] = best == gs.best_params_
    return res, X, y


def event_ms(call, reps):
    """HIP-event times of ``call`` after one warm-up"""
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def run_masks(rml, N, segments, jobs, solver, refit, reps, seed):
    """ProjMaskSearchSVC against the seven GridSearchSVC fits on column subsets that it replaces, alternating, same options"""
    import torch
    from sklearn.model_selection import StratifiedKFold
    import radar_ml_amd.train as T
    Dm = sum(segments)
    X, y = synth(N, True, seed, Dm)
    masks = T._all_proj_masks()
    start = np.concatenate([[0], np.cumsum(segments)])
    cols = [np.concatenate([np.arange(start[i], start[i + 1]) for i in range(3) if m[i]]) for m in masks]
    subsets = [np.ascontiguousarray(X[:, c]) for c in cols]          # the loop's inputs, made outside its clock
    kw = dict(n_jobs=max(jobs), solver=solver, refit_solver=refit)
    cv = lambda: StratifiedKFold(5).split(X, y)

    def mask_search():
        return T.ProjMaskSearchSVC(base_svc(), GRID, segments, cv=cv(), **kw).fit(X, y)

    def loop():
        fits = [T.GridSearchSVC(base_svc(), GRID, cv=cv(), **kw).fit(Xs, y) for Xs in subsets]
        return max(enumerate(fits), key=lambda f: (f[1].best_score_, -f[0]))

    seen = []
    real = T._smo_masks

    def watched(Xh, seg, keys, plan, device=None):
        out = real(Xh, seg, keys, plan, device)
        seen.append((len(plan["problems"]), out["solve_s"], out["score_s"]))
        return out
    T._smo_masks = watched
    try:
        ms, (wi, w) = mask_search(), loop()                           # warm-up of both (code load, workspace growth)
        t_mask, t_loop = [], []
        for r in range(reps):
            del seen[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms = mask_search()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            wi, w = loop()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_mask.append(t1 - t0)
            t_loop.append(t2 - t1)
            progress("rep %d: mask search %.3f s, seven-search loop %.3f s" % (r, t1 - t0, t2 - t1))
    finally:
        T._smo_masks = real
    if solver == "device":
        solve_ms, score_ms = 1e3 * sum(s[1] for s in seen), 1e3 * sum(s[2] for s in seen)
    else:
        n_splits = ms.n_splits_
        solve_ms = 1e3 * float(ms.cv_results_["mean_fit_time"].sum()) * n_splits
        score_ms = 1e3 * float(ms.cv_results_["mean_score_time"].sum()) * n_splits
    # the two kernels' own time: HIP events around the calls on resident rows
    Xd = torch.from_numpy(X).cuda()
    keys = [(b,) + k for b in range(1, 8) for k in [("linear", None)] + [("rbf", float(g)) for g in GAMMAS]]
    G, nsq = T.segment_products_device(Xd, segments)
    seg_ms = event_ms(lambda: T.segment_products_device(Xd, segments), reps)
    cmp_ms = event_ms(lambda: T.compose_device(G, nsq, keys), reps)
    # ... beside rml_gram of ONE mask (all columns, the six kernels), what each of the loop's seven searches starts with
    from radar_ml_amd import _lib
    kinds = np.array([_lib.GRAM_LINEAR] + [_lib.GRAM_RBF] * len(GAMMAS), dtype=np.int32)
    gammas = np.array([0.0] + [float(g) for g in GAMMAS], dtype=np.float64)
    out6 = torch.empty((6, N, N), dtype=torch.float64, device="cuda")
    one_ms = event_ms(lambda: _lib.check(_lib.load().rml_gram(_lib.context(), _lib.ptr(Xd), Dm, N, Dm, 6, kinds.ctypes.data,
                                                              gammas.ctypes.data, _lib.ptr(out6), N, N * N, _lib.stream_ptr()),
                                         "rml_gram"), reps)
    res = {"rows": N, "segments": list(segments), "D": Dm, "masks": 7, "matrices": len(keys), "solver": solver, "refit_solver": refit,
           "n_jobs": max(jobs), "reps": reps,
           "mask_search_s": round(float(np.median(t_mask)), 4), "loop_s": round(float(np.median(t_loop)), 4),
           "mask_search_s_all": [round(t, 4) for t in t_mask], "loop_s_all": [round(t, 4) for t in t_loop],
           "gram_segments_ms": round(float(np.median(seg_ms)), 3), "compose_ms": round(float(np.median(cmp_ms)), 3),
           "gram_segments_ms_all": [round(t, 3) for t in seg_ms], "compose_ms_all": [round(t, 3) for t in cmp_ms],
           "rml_gram_one_mask_ms": round(float(np.median(one_ms)), 3),
           "solve_ms": round(solve_ms, 2), "score_ms": round(score_ms, 2), "refit_s": round(ms.refit_time_, 4),
           "best_proj_mask": list(ms.best_proj_mask_), "best_params": ms.best_params_, "best_score": round(ms.best_score_, 4),
           "loop_best_proj_mask": list(masks[wi]), "loop_best_params": w.best_params_, "loop_best_score": round(w.best_score_, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1458,7290", help="training set sizes to run (1458: code grid, 7290: off-grid)")
    ap.add_argument("--jobs", default="4,16", help="n_jobs values of the host search")
    ap.add_argument("--solver", default="host", choices=["host", "device"], help="where the search's SVC duals are solved")
    ap.add_argument("--refit", default="host", choices=["host", "device"], help="where the winner is refitted (refit_s)")
    ap.add_argument("--sklearn", action="store_true", help="also time scikit-learn's GridSearchCV on the 1458 set (sub-grid)")
    ap.add_argument("--masks", action="store_true", help="time the projection-mask search against the seven-search loop it replaces")
    ap.add_argument("--segments", default="3872,5457,682", help="--masks: the xz, yz, xy feature counts of the synthetic rows")
    ap.add_argument("--reps", type=int, default=5, help="--masks: repeats of each side (medians are reported)")
    args = ap.parse_args()
    import torch
    import radar_ml_amd as rml
    assert torch.cuda.is_available(), "needs a GPU"
    jobs = [int(j) for j in args.jobs.split(",")]
    t_all = time.perf_counter()
    if args.masks:
        n = int(args.sets.split(",")[0])
        out = {"metric": "svc_proj_mask_search", "grid": "7 masks x (5 linear + 25 rbf), 5 folds"}
        out.update(run_masks(rml, n, tuple(int(v) for v in args.segments.split(",")), jobs, args.solver, args.refit, args.reps, seed=n))
        out["wall_s"] = round(time.perf_counter() - t_all, 1)
        print(json.dumps(out))
        return
    out = {"metric": "svc_grid_search", "grid": "5 linear + 25 rbf, 5 folds", "f64_peak_tflops": F64_PEAK / 1e12, "sets": []}
    keep = None
    for n in [int(s) for s in args.sets.split(",")]:
        r, X, y = (run_set_device if args.solver == "device" else run_set)(rml, n, n == 1458, jobs, seed=n, refit=args.refit)
        out["sets"].append(r)
        if n == 1458:
            keep = (X, y)
    if args.sklearn and keep is not None:
        from sklearn.model_selection import GridSearchCV, StratifiedKFold
        X, y = keep
        j = max(jobs)
        t0 = time.perf_counter()
        ref = GridSearchCV(base_svc(), SUB_GRID, n_jobs=j, cv=StratifiedKFold(5).split(X, y)).fit(X, y)
        t_sk = time.perf_counter() - t0
        progress("scikit-learn GridSearchCV on the sub-grid: %.1f s" % t_sk)
        t0 = time.perf_counter()
        ours = rml.GridSearchSVC(base_svc(), SUB_GRID, n_jobs=j, cv=StratifiedKFold(5).split(X, y)).fit(X, y)
        t_ours = time.perf_counter() - t0
        same_splits = all(np.array_equal(ours.cv_results_["split%d_test_score" % k], ref.cv_results_["split%d_test_score" % k])
                          for k in range(5))
        out["sklearn"] = {"rows": int(X.shape[0]), "grid": "C {1, 10} linear + C {1, 10} x gamma {0.001, 0.01} rbf, 5 folds",
                          "n_jobs": j, "sklearn_s": round(t_sk, 2), "gridsearchsvc_s": round(t_ours, 2),
                          "speedup": round(t_sk / t_ours, 1), "best_params_agree": ours.best_params_ == ref.best_params_,
                          "split_scores_identical": bool(same_splits), "best_params": ref.best_params_}
    out["wall_s"] = round(time.perf_counter() - t_all, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
