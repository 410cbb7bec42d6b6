"""Shared by test_sgd_cpu.py and test_sgd_gpu.py: a NumPy twin of csrc/sgd.hip (scikit-learn 1.7.2's ``_plain_sgd64`` for
``loss='log_loss'``, ``learning_rate='optimal'``, dense rows) with a pluggable order of the dot product, the cases, and their seeded
generators.  References are computed once per process and shared."""
import functools
import math

import numpy as np

MAX_INT = np.iinfo(np.int32).max
L1, L2, ELASTICNET = 1, 2, 3
PENALTY = {"l1": L1, "l2": L2, "elasticnet": ELASTICNET}
THREADS, WAVE = 1024, 64

# the case grid of the kernel tests (SGDClassifier keywords)
CASES = {
    "l2_1e-3": dict(penalty="l2", alpha=1e-3),
    "l1_1e-4": dict(penalty="l1", alpha=1e-4),
    "en_1e-5": dict(penalty="elasticnet", alpha=1e-5, l1_ratio=0.15),
    "l2_1e-7_avg": dict(penalty="l2", alpha=1e-7, average=True),
    "en_1e-8_avg": dict(penalty="elasticnet", alpha=1e-8, l1_ratio=0.3, average=True),
    "l2_10": dict(penalty="l2", alpha=10.0),
}
RANDOM_STATE = 1


def make_rows(n, D, n_classes=3, noise=0.6, seed=0):
    """Rows that are codes k / 255 in float32 with about 60 % zeros, in ``n_classes`` overlapping classes."""
    rng = np.random.RandomState(seed)
    y = np.arange(n) % n_classes
    rng.shuffle(y)
    centres = rng.rand(n_classes, D)
    v = centres[y] + noise * rng.randn(n, D)
    v = np.clip(v, 0.0, 1.0)
    v[rng.rand(n, D) < 0.6] = 0.0
    X = (np.round(v * 255.0).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    return X, y.astype(np.int64)


# ---- the dot orders ----------------------------------------------------------------------------------------------------------
def dot_sequential(w, x):
    """scikit-learn's: innerprod += w[j] * x[j], j ascending (np.add.accumulate is strictly sequential)."""
    return float(np.add.accumulate(w * x)[-1]) if len(w) else 0.0


def _strided(w, x, lanes):
    """Per-lane sums: lane t adds the products of the elements t, t + lanes, .. in ascending order, from 0."""
    D = len(w)
    nk = -(-D // lanes)
    prod = np.zeros(nk * lanes)
    prod[:D] = w * x
    prod = prod.reshape(nk, lanes)
    s = np.zeros(lanes)
    for k in range(nk):
        m = min(lanes, D - k * lanes)               # lanes past D add nothing (not even a zero)
        s[:m] = s[:m] + prod[k, :m]
    return s


_LANE = np.arange(THREADS)


def dot_kernel(w, x):
    """The order csrc/sgd.hip documents: 1 024 strided thread sums, a butterfly within each wave of 64, the 16 wave sums in order."""
    s = _strided(w, x, THREADS)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[_LANE ^ m]
    tot = s[0]
    for v in range(1, THREADS // WAVE):
        tot = tot + s[v * WAVE]
    return float(tot)


def dot_tree256(w, x):
    """Another plausible order: 256 strided sums, then a binary tree over neighbours."""
    s = _strided(w, x, 256)
    while len(s) > 1:
        s = s[0::2] + s[1::2]
    return float(s[0])


DOTS = {"sequential": dot_sequential, "kernel": dot_kernel, "tree256": dot_tree256}


# ---- the twin ------------------------------------------------------------------------------------------------------------------
def our_rand_r(seed):
    if seed == 0:
        seed = 1
    seed ^= (seed << 13) & 0xFFFFFFFF
    seed ^= seed >> 17
    seed ^= (seed << 5) & 0xFFFFFFFF
    return seed, seed % (2 ** 31)


def shuffle_inplace(ind, seed):
    n = len(ind)
    for i in range(n - 1):
        seed, r = our_rand_r(seed)
        j = i + r % (n - i)
        ind[i], ind[j] = ind[j], ind[i]


def log1pexp(x):
    if x <= -37:
        return math.exp(x)
    if x <= -2:
        return math.log1p(math.exp(x))
    if x <= 18:
        return math.log(1. + math.exp(x))
    if x <= 33.3:
        return x + math.exp(-x)
    return x


def gradient(y, p):
    if p > -37:
        e = math.exp(-p)
        return ((1 - y) - y * e) / (1 + e)
    return math.exp(p) - y


def optimal_init(alpha):
    typw = np.sqrt(1.0 / np.sqrt(alpha))
    return 1.0 / ((typw / max(1.0, gradient(1.0, -typw))) * alpha)


def plain_sgd(X, y, penalty, alpha, l1_ratio=0.15, average=0, max_iter=1000, tol=1e-3, n_iter_no_change=5, shuffle=True, seed=0,
              weight_pos=1.0, weight_neg=1.0, t0=1.0, init=None, order="sequential", margins=None):
    """``_plain_sgd64`` on the float64 rows ``X`` (dataset order) and labels ``y`` (0 / 1).  ``init``: (coef, intercept, avg_coef,
    avg_intercept) of a warm start.  ``margins``: a list that receives |sumloss - (best_loss - tol n)| of every epoch's stopping
    comparison.  Returns a dict of coef, intercept, avg_coef, avg_intercept, n_iter, t, status."""
    dot = DOTS[order]
    n, D = X.shape
    ptype = PENALTY[penalty] if isinstance(penalty, str) else penalty
    average = int(average)
    w = np.zeros(D)
    aw = np.zeros(D)
    intercept = avg_intercept = 0.0
    if init is not None:
        w, intercept = np.array(init[0], dtype=np.float64), float(init[1])
        if average > 0:
            aw, avg_intercept = np.array(init[2], dtype=np.float64), float(init[3])
    q = np.zeros(D)
    tol = -np.inf if tol is None else float(tol)
    l1_ratio = 0.0 if ptype == L2 else (1.0 if ptype == L1 else float(l1_ratio))
    opt_init = optimal_init(alpha)
    wscale, average_a, average_b, u, t = 1.0, 0.0, 1.0, 0.0, float(t0)
    best_loss, no_improvement, status, epochs = np.inf, 0, 1, 0
    ind = list(range(n))

    def reset():
        nonlocal w, aw, wscale, average_a, average_b
        if average > 0:
            aw = aw + average_a * w
            aw = aw * (1.0 / average_b)
            average_a, average_b = 0.0, 1.0
        w = w * wscale
        wscale = 1.0

    with np.errstate(all="ignore"):
        for epoch in range(int(max_iter)):
            sumloss = 0.0
            if shuffle:
                shuffle_inplace(ind, int(seed))
            for i in range(n):
                x, yi = X[ind[i]], float(y[ind[i]])
                p = dot(w, x) * wscale + intercept
                eta = 1.0 / (alpha * (opt_init + t - 1))
                sumloss += log1pexp(p) - yi * p
                cw = weight_pos if yi > 0.0 else weight_neg
                dloss = min(max(gradient(yi, p), -1e12), 1e12)
                update = -eta * dloss
                update *= cw * 1.0
                if ptype >= L2:
                    wscale *= max(0, 1.0 - ((1.0 - l1_ratio) * eta * alpha))
                    if wscale < 1e-9:
                        reset()
                if update != 0.0:
                    w = w + x * (update / wscale)
                    intercept += update * 1.0
                if 0 < average <= t:
                    num_iter = t - average + 1
                    aw = aw + average_a * x * (-update / wscale)
                    mu = 1.0 / num_iter
                    if num_iter > 1:
                        average_b /= (1.0 - mu)
                    average_a += mu * average_b * wscale
                    avg_intercept += ((intercept - avg_intercept) / num_iter)
                if ptype in (L1, ELASTICNET):
                    u += (l1_ratio * eta * alpha)
                    z = w
                    pos, neg = wscale * z > 0.0, wscale * z < 0.0
                    w = np.where(pos, np.maximum(0.0, z - ((u + q) / wscale)), np.where(neg, np.minimum(0.0, z + ((u - q) / wscale)), z))
                    q = q + wscale * (w - z)
                t += 1
            epochs = epoch + 1
            if not (np.isfinite(intercept) and np.isfinite(w).all()):
                status = 2
                break
            if margins is not None and tol > -np.inf and np.isfinite(best_loss):
                margins.append(abs(sumloss - (best_loss - tol * n)))
            if tol > -np.inf and sumloss > best_loss - tol * n:
                no_improvement += 1
            else:
                no_improvement = 0
            if sumloss < best_loss:
                best_loss = sumloss
            if no_improvement >= n_iter_no_change:
                status = 0
                break
    if status != 2:
        reset()
    return dict(coef=w, intercept=intercept, avg_coef=aw, avg_intercept=avg_intercept, n_iter=epochs, t=float(t0) + epochs * n,
                status=status)


def shuffle_seeds(random_state, n_classes):
    """The shuffle seed of every binary problem of ``SGDClassifier(random_state=...).fit`` (an independent restatement of
    _fit_binary / _fit_multiclass / fit_binary / make_dataset): one for two classes, else one per class."""
    if n_classes == 2:
        rs = np.random.RandomState(random_state)
        rs.randint(1, MAX_INT)
        return [int(rs.randint(MAX_INT))]
    out = []
    for s in np.random.RandomState(random_state).randint(MAX_INT, size=n_classes):
        rs = np.random.RandomState(s)
        rs.randint(1, MAX_INT)
        out.append(int(rs.randint(MAX_INT)))
    return out


def twin_fit(X32, y, order="sequential", random_state=RANDOM_STATE, margins=None, **kw):
    """``SGDClassifier(loss='log_loss', random_state=..., **kw).fit`` by the twin.  Returns a dict of the estimator's
    ``coef`` (n_dec, D), ``intercept``, ``n_iter`` per problem, ``t`` and the per-problem results ``probs``."""
    X64 = X32.astype(np.float64)
    classes = np.unique(y)
    nc = len(classes)
    positives = [1] if nc == 2 else range(nc)
    seeds = shuffle_seeds(random_state, nc)
    average = int(kw.get("average", 0))
    args = {k: v for k, v in kw.items() if k != "average"}
    probs = [plain_sgd(X64, (y == classes[c]).astype(np.float64), average=average, seed=s, order=order, margins=margins, **args)
             for c, s in zip(positives, seeds)]
    t = 1.0 + max(p["n_iter"] for p in probs) * len(y)
    avg = average > 0 and average <= t - 1
    return dict(coef=np.array([p["avg_coef"] if avg else p["coef"] for p in probs]),
                intercept=np.array([p["avg_intercept"] if avg else p["intercept"] for p in probs]),
                n_iter=[p["n_iter"] for p in probs], t=t, probs=probs, classes=classes)


def sklearn_fit(X32, y, random_state=RANDOM_STATE, **kw):
    from sklearn.linear_model import SGDClassifier
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return SGDClassifier(loss="log_loss", random_state=random_state, **kw).fit(X32.astype(np.float64), y)


def scaled_err(got_coef, got_icpt, want_coef, want_icpt):
    """max |difference| of coefficients and intercepts over max |coef|."""
    scale = float(np.abs(want_coef).max()) or 1.0
    return max(float(np.abs(np.asarray(got_coef) - want_coef).max()), float(np.abs(np.asarray(got_icpt) - want_icpt).max())) / scale


# ---- the data sets of the kernel tests (name -> rows, labels); every case of CASES runs on "main" ------------------------------
@functools.lru_cache(maxsize=None)
def dataset(name):
    if name == "main":
        return make_rows(150, 640, seed=0)
    if name == "d96":
        return make_rows(150, 96, seed=1)
    if name == "d1030":
        return make_rows(150, 1030, seed=2)
    if name == "n60":
        return make_rows(60, 640, seed=3)
    if name == "bin":
        return make_rows(40, 96, n_classes=2, seed=4)
    raise KeyError(name)


# (data set, case) pairs beside the full grid on "main"
EXTRA = [("d96", "l2_1e-3"), ("d96", "en_1e-8_avg"), ("d1030", "l1_1e-4"), ("d1030", "l2_1e-7_avg"), ("n60", "en_1e-5"),
         ("n60", "l2_1e-7_avg"), ("bin", "l2_1e-3"), ("bin", "en_1e-8_avg")]
PAIRS = [("main", c) for c in CASES] + EXTRA


def est_problems(est):
    """The per-problem standard / averaged weights and intercepts of a fitted SGDClassifier, as the solver's outputs hold them."""
    K = est.coef_.shape[0]
    avg = est.average > 0
    sc = (est._standard_coef if avg else est.coef_).reshape(K, -1)
    si = est._standard_intercept if avg else est.intercept_
    ac = est._average_coef.reshape(K, -1) if avg else np.zeros_like(sc)
    ai = est._average_intercept if avg else np.zeros(K)
    return [dict(coef=sc[k], intercept=si[k], avg_coef=ac[k], avg_intercept=ai[k]) for k in range(K)]


def deviation(probs, want, scale):
    """max |difference| over the problems' weights and intercepts (standard and averaged), over ``scale``."""
    return max(max(np.abs(p["coef"] - w["coef"]).max(), abs(p["intercept"] - w["intercept"]), np.abs(p["avg_coef"] - w["avg_coef"]).max(),
                   abs(p["avg_intercept"] - w["avg_intercept"])) for p, w in zip(probs, want)) / scale


def make_reference(X, y, kw):
    est = sklearn_fit(X, y, **kw)
    want = est_problems(est)
    scale = float(np.abs(est.coef_).max()) or 1.0
    tk = twin_fit(X, y, order="kernel", **kw)
    tt = twin_fit(X, y, order="tree256", **kw)
    delta = max(deviation(tk["probs"], want, scale), deviation(tt["probs"], want, scale))
    return dict(est=est, kernel=tk, scale=scale, delta=delta, tol=max(8 * delta, 1e-12))


@functools.lru_cache(maxsize=None)
def reference(data, case):
    """scikit-learn's fit of a (data set, case) pair; the twin's in the kernel's order; delta: the larger deviation from scikit-learn
    of the twin in 'kernel' and in 'tree256' order, over max|coef_| -- what a change of the summation order alone does to this
    case; and the tolerance max(8 delta, 1e-12) of the GPU tests.  Computed once."""
    X, y = dataset(data)
    return make_reference(X, y, CASES[case])


# ---- the device hook of radar_ml_amd.train replaced by the twin ---------------------------------------------------------------
def twin_device(X32, plan, order="sequential", gaps=None):
    """What ``train.sgd_device`` returns for ``plan`` on the host rows ``X32``, computed by the twin.  ``gaps``: a list that
    receives every held-out row's top-two decision gap (|dec| for two classes)."""
    X64 = np.asarray(X32, dtype=np.float32).astype(np.float64)
    D = X64.shape[1]
    probs, n_out = plan["problems"], int(plan["n_out"])
    coef, avg_coef = np.zeros((n_out, D)), np.zeros((n_out, D))
    icpt, avg_icpt, n_iter, t, status = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, np.int32), np.zeros(n_out), np.zeros(n_out, np.int32)
    init = plan.get("init")
    for p in probs:
        o, n = int(p["out"]), int(p["n"])
        rows = plan["rows"][int(p["rows_off"]):int(p["rows_off"]) + n]
        y = plan["y"][int(p["y_off"]):int(p["y_off"]) + n]
        start = (init["coef"][o], init["intercept"][o], init["avg_coef"][o], init["avg_intercept"][o]) if p["warm"] else None
        r = plain_sgd(X64[rows], y.astype(np.float64), int(p["penalty"]), float(p["alpha"]), float(p["l1_ratio"]), int(p["average"]),
                      int(p["max_iter"]), float(p["tol"]), int(p["n_iter_no_change"]), bool(p["shuffle"]), int(p["seed"]),
                      float(p["weight_pos"]), float(p["weight_neg"]), float(p["t0"]), start, order)
        coef[o], avg_coef[o], icpt[o], avg_icpt[o] = r["coef"], r["avg_coef"], r["intercept"], r["avg_intercept"]
        n_iter[o], t[o], status[o] = r["n_iter"], r["t"], r["status"]
    C = int(plan.get("n_classes", 2))
    n_dec = 1 if C == 2 else C
    fits = plan.get("fits", [])
    n_test = len(plan.get("test_rows", []))
    dec, labels, correct = np.zeros((n_test, n_dec)), np.zeros(n_test, np.int32), np.zeros(len(fits), np.int32)
    for f, F in enumerate(fits):
        ps = probs[int(F["prob0"]):int(F["prob0"]) + n_dec]
        tfit = max(t[int(p["out"])] for p in ps)
        sl = slice(int(F["test_off"]), int(F["test_off"]) + int(F["n_test"]))
        for c, p in enumerate(ps):
            avg = p["average"] > 0 and p["average"] <= tfit - 1
            cf, b = (avg_coef, avg_icpt) if avg else (coef, icpt)
            for r, row in zip(range(sl.start, sl.stop), plan["test_rows"][sl]):
                dec[r, c] = DOTS[order](cf[int(p["out"])], X64[row]) + b[int(p["out"])]
        labels[sl] = (dec[sl, 0] > 0).astype(np.int32) if C == 2 else dec[sl].argmax(axis=1)
        correct[f] = int((labels[sl] == plan["test_y"][sl]).sum())
        if gaps is not None:
            srt = np.sort(dec[sl], axis=1)
            gaps.extend(np.abs(dec[sl, 0]) if C == 2 else srt[:, -1] - srt[:, -2])
    return {"intercept": icpt, "avg_intercept": avg_icpt, "n_iter": n_iter, "t": t, "status": status, "dec": dec, "labels": labels,
            "correct": correct, "solve_s": 0.0, "score_s": 0.0, "coefs": lambda slots: (coef[list(slots)], avg_coef[list(slots)])}


def twin_hook(order="sequential", gaps=None, calls=None):
    """A replacement for ``train._sgd``."""
    def hook(X, plan, device=None):
        if calls is not None:
            calls.append(plan)
        out = twin_device(X, plan, order, gaps)
        out["solve"] = lambda plan2: hook(X, plan2)
        return out
    return hook


# the small search of the tests: a 2 x 2 grid, 3 folds
SEARCH_GRID = {"alpha": [1e-3, 1e-5], "penalty": ["l2", "elasticnet"]}
SEARCH_CV = 3


def search_rows():
    return make_rows(120, 640, seed=5)


@functools.lru_cache(maxsize=None)
def sklearn_search():
    import warnings
    from sklearn.linear_model import SGDClassifier
    from sklearn.model_selection import GridSearchCV
    X, y = search_rows()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return GridSearchCV(SGDClassifier(loss="log_loss", random_state=RANDOM_STATE), SEARCH_GRID, cv=SEARCH_CV).fit(X.astype(np.float64), y)


def check_search(gs):
    """``gs`` (a fitted GridSearchSGD) against GridSearchCV(SGDClassifier) on the same rows: scores, ranks, best_params_ equal."""
    ref = sklearn_search()
    assert gs.cv_results_["params"] == ref.cv_results_["params"]
    for key in ["split%d_test_score" % s for s in range(SEARCH_CV)] + ["mean_test_score", "std_test_score", "rank_test_score"]:
        np.testing.assert_array_equal(gs.cv_results_[key], ref.cv_results_[key], err_msg=key)
    assert gs.best_params_ == ref.best_params_ and gs.best_index_ == ref.best_index_ and gs.best_score_ == ref.best_score_
    assert set(gs.cv_results_) == set(ref.cv_results_)
    return ref


# ---- plans for train.sgd_device, and references for problems scikit-learn's fit() cannot pose ---------------------------------
def make_plan(T, fits, n_classes, test=None):
    """A plan of ``fits``: a list of (rows, y01 lists (one per problem), seeds, SGDClassifier keywords); problem slots in order.
    ``test``: per fit (held-out rows, class indices) or None."""
    from sklearn.linear_model import SGDClassifier
    problems, rows, ys, pf, te_rows, te_y = [], [], [], [], [], []
    n_rows = n_y = n_test = 0
    for f, (rr, ylists, seeds, kw) in enumerate(fits):
        prm = T._sgd_params(SGDClassifier(loss="log_loss", **kw).get_params(), "test")
        if test is not None:
            pf.append((len(problems), len(test[f][0]), n_test))
            te_rows.append(test[f][0]); te_y.append(test[f][1])
            n_test += len(test[f][0])
        for yl, seed in zip(ylists, seeds):
            problems.append(T._sgd_problem(prm, len(rr), seed, n_rows, n_y, len(problems), 1.0, 1.0))
            ys.append(yl)
            n_y += len(rr)
        rows.append(rr)
        n_rows += len(rr)
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return {"problems": np.array(problems, dtype=T.SGD_PROBLEM), "rows": cat(rows), "y": cat(ys), "n_out": len(problems),
            "fits": np.array(pf, dtype=T.SGD_FIT), "test_rows": cat(te_rows), "test_y": cat(te_y), "n_classes": n_classes}


def class_fit(X, y, case, random_state=RANDOM_STATE):
    """(rows, label lists, seeds, keywords) of SGDClassifier(random_state, **CASES[case]).fit(X, y) for make_plan."""
    classes = np.unique(y)
    positives = [1] if len(classes) == 2 else range(len(classes))
    return (np.arange(len(y)), [(y == classes[c]).astype(np.int32) for c in positives], shuffle_seeds(random_state, len(classes)),
            CASES[case] if isinstance(case, str) else case)


def check_problem(out, slot, coefs, want, scale, tol, what):
    """One solved problem of a sgd_device result against a twin result ``want`` (kernel order): n_iter, t, status equal, weights and
    intercepts within tol * scale.  Returns the error over scale."""
    coef, avg_coef = coefs
    assert out["n_iter"][slot] == want["n_iter"] and out["t"][slot] == want["t"] and out["status"][slot] == want["status"], what
    err = max(np.abs(coef - want["coef"]).max(), abs(out["intercept"][slot] - want["intercept"]),
              np.abs(avg_coef - want["avg_coef"]).max(), abs(out["avg_intercept"][slot] - want["avg_intercept"])) / scale
    assert err <= tol, "%s: error %.3g over max|coef| against the twin, tolerance %.3g" % (what, err, tol)
    return err


def twin_problem(X32, rows, y01, seed, kw, order):
    args = {k: v for k, v in kw.items()}
    args["average"] = int(args.get("average", 0))
    return plain_sgd(X32[rows].astype(np.float64), np.asarray(y01, dtype=np.float64), seed=seed, order=order, **args)


def twin_reference(X32, rows, y01, seed, kw):
    """For a problem scikit-learn's fit() cannot pose (a class without rows, a row subset with its own seed): the twin in
    scikit-learn's order stands for scikit-learn (test_sgd_cpu.py holds the two equal), delta is formed as in ``reference``."""
    seq, ker, tree = (twin_problem(X32, rows, y01, seed, kw, o) for o in ("sequential", "kernel", "tree256"))
    scale = max(float(np.abs(seq["coef"]).max()), float(np.abs(seq["avg_coef"]).max())) or 1.0
    dev = lambda r: max(np.abs(r["coef"] - seq["coef"]).max(), abs(r["intercept"] - seq["intercept"]),
                        np.abs(r["avg_coef"] - seq["avg_coef"]).max(), abs(r["avg_intercept"] - seq["avg_intercept"])) / scale
    delta = max(dev(ker), dev(tree))
    return dict(kernel=ker, scale=scale, delta=delta, tol=max(8 * delta, 1e-12))
