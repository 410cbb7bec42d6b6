"""SVC hyperparameter search of the reference's ``train.py`` (``find_best_svm_estimator``, train.py:462-491) on GPU kernel matrices.

The reference runs ``GridSearchCV(SVC(probability=True, class_weight='balanced'))`` over 5 linear and 25 RBF points with 5 folds;
libsvm spends nearly all of that time computing kernel values one pair at a time.  ``GridSearchSVC`` computes the inner products of
the training rows once on the GPU (``rml_gram``, csrc/gram.hip), writes every kernel matrix the grid needs from them, and fits
libsvm's ``SVC(kernel='precomputed')`` on slices of those matrices -- the same fits, on the same kernel values to the last few ulps.
The winner comes back as a genuine ``sklearn.svm.SVC`` with kernel ``rbf`` or ``linear``, so everything after the search in the
reference (``CalibratedClassifierCV(cv='prefit')``, the pickle, predict.py, ``from_sklearn``) works on it unchanged.
"""
import logging
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

_GRID_KEYS = ("C", "kernel", "gamma")
# SVC constructor parameters that carry from the base estimator into every fit
_CARRY = ("C", "probability", "class_weight", "random_state", "cache_size", "tol", "shrinking", "max_iter",
          "decision_function_shape", "break_ties")
_NONFINITE = "Input contains NaN, infinity or a value too large for dtype('float64')."      # scikit-learn's message


def _gram_device(X, kernels, dev):
    """``rml_gram`` of the float32 host rows ``X`` for ``kernels``: a DEVICE (len(kernels), N, N) float64 tensor."""
    import torch
    lib = _lib.load()
    if not 1 <= len(kernels) <= 8:
        raise ValueError("_gram: 1..8 kernels per call, got %d" % len(kernels))
    N, D = X.shape
    ctx = _lib.context(dev)
    kinds = np.array([_lib.GRAM_LINEAR if k == "linear" else _lib.GRAM_RBF for k, _ in kernels], dtype=np.int32)
    gammas = np.array([0.0 if g is None else float(g) for _, g in kernels], dtype=np.float64)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    out = torch.empty((len(kernels), N, N), dtype=torch.float64, device=dev)
    _lib.check(lib.rml_gram(ctx, _lib.ptr(Xd), D, N, D, len(kernels), kinds.ctypes.data, gammas.ctypes.data, _lib.ptr(out),
                            N, N * N, _lib.stream_ptr(dev)), "rml_gram")
    return out


def _gram(X, kernels, device=None):
    """Every kernel matrix of ``kernels`` (a list of ('linear', None) / ('rbf', gamma), at most 8) of the float32 rows ``X`` against
    themselves: one upload, one ``rml_gram`` call, one copy back.  Returns a list of host (N, N) float64 matrices.

    All device work of the host search goes through this function (tests replace it to run the search logic without a GPU)."""
    import torch
    dev = _lib.device_of(device)
    with torch.cuda.device(dev):
        host = _gram_device(X, kernels, dev).cpu().numpy()
    return [host[k] for k in range(len(kernels))]


# rml_smo_problem / rml_smo_fit of include/radarml.h
SMO_PROBLEM = np.dtype([("matrix", "<i4"), ("l", "<i4"), ("n_pos", "<i4"), ("shrinking", "<i4"), ("max_iter", "<i4"), ("reserved", "<i4"),
                        ("rows_off", "<i8"), ("alpha_off", "<i8"), ("Cp", "<f8"), ("Cn", "<f8"), ("eps", "<f8")])
SMO_FIT = np.dtype([("prob0", "<i4"), ("n_test", "<i4"), ("test_off", "<i8")])


def smo_device(Kd, plan, device=None):
    """``rml_smo_solve`` + ``rml_smo_score`` on the DEVICE matrices ``Kd`` (a (nk, N, N) float64 tensor, each matrix bit-exactly
    symmetric) for ``plan``: a dict of ``problems`` (SMO_PROBLEM records), ``rows`` (int32, the problems' Gram rows), ``fits``
    (SMO_FIT records), ``test_rows`` / ``test_y`` (int32: held-out Gram rows and their class indices) and ``n_classes``.
    Returns host arrays ``alpha``, ``rho``, ``n_iter``, ``stopped`` per problem, ``dec``, ``labels`` per held-out row, ``correct`` per
    fit, and ``solve_s`` / ``score_s``, the wall time of the two batched calls."""
    import torch
    lib = _lib.load()
    dev = _lib.device_of(device if device is not None else Kd.device)
    ctx = _lib.context(dev)
    probs = np.ascontiguousarray(plan["problems"], dtype=SMO_PROBLEM)
    fits = np.ascontiguousarray(plan["fits"], dtype=SMO_FIT)
    nk, N = int(Kd.shape[0]), int(Kd.shape[1])
    if Kd.dtype != torch.float64 or Kd.dim() != 3 or Kd.shape[2] != N or not Kd.is_contiguous():
        raise ValueError("smo_device: the matrices are a contiguous (nk, N, N) float64 tensor")
    C = int(plan["n_classes"])
    P = C * (C - 1) // 2
    n_alpha = int((probs["alpha_off"] + probs["l"]).max()) if len(probs) else 0
    with torch.cuda.device(dev):
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        rows, te_rows, te_y = i32(plan["rows"]), i32(plan["test_rows"]), i32(plan["test_y"])
        n_test = int(te_rows.numel())
        alpha = torch.zeros(max(n_alpha, 1), dtype=torch.float64, device=dev)
        rho = torch.zeros(max(len(probs), 1), dtype=torch.float64, device=dev)
        n_iter = torch.zeros(max(len(probs), 1), dtype=torch.int32, device=dev)
        stopped = torch.zeros(max(len(probs), 1), dtype=torch.int32, device=dev)
        dec = torch.zeros(max(n_test * P, 1), dtype=torch.float64, device=dev)
        labels = torch.zeros(max(n_test, 1), dtype=torch.int32, device=dev)
        correct = torch.zeros(max(len(fits), 1), dtype=torch.int32, device=dev)
        st = _lib.stream_ptr(dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        _lib.check(lib.rml_smo_solve(ctx, _lib.ptr(Kd), N, N, N * N, nk, probs.ctypes.data, len(probs), _lib.ptr(rows), int(rows.numel()),
                                     _lib.ptr(alpha), n_alpha, _lib.ptr(rho), _lib.ptr(n_iter), _lib.ptr(stopped), st), "rml_smo_solve")
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        _lib.check(lib.rml_smo_score(ctx, _lib.ptr(Kd), N, N, N * N, nk, probs.ctypes.data, len(probs), _lib.ptr(rows), int(rows.numel()),
                                     _lib.ptr(alpha), n_alpha, _lib.ptr(rho), C, fits.ctypes.data, len(fits), _lib.ptr(te_rows),
                                     _lib.ptr(te_y), n_test, _lib.ptr(dec), _lib.ptr(labels), _lib.ptr(correct), st), "rml_smo_score")
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        out = {"alpha": alpha.cpu().numpy()[:n_alpha], "rho": rho.cpu().numpy()[:len(probs)], "n_iter": n_iter.cpu().numpy()[:len(probs)],
               "stopped": stopped.cpu().numpy()[:len(probs)], "dec": dec.cpu().numpy()[:n_test * P].reshape(n_test, P),
               "labels": labels.cpu().numpy()[:n_test], "correct": correct.cpu().numpy()[:len(fits)],
               "solve_s": t1 - t0, "score_s": t2 - t1}
    if (out["stopped"] < 0).any():
        raise _lib.RadarMLError("rml_smo_solve: a problem names a row outside the matrix")
    if (out["labels"] < 0).any():
        raise _lib.RadarMLError("rml_smo_score: a held-out row outside the matrix")
    return out


def _smo(X, kernels, plan, device=None):
    """The kernel matrices of ``kernels`` of the float32 rows ``X`` (``rml_gram``, as ``_gram``) kept ON THE DEVICE, every dual of
    ``plan`` solved on them in one ``rml_smo_solve`` call and every held-out row scored in one ``rml_smo_score`` call (``smo_device``).
    Returns ``smo_device``'s dict plus ``matrix``: a function k -> host copy of matrix k (the search fetches the winner's only), and
    ``solve``: a function plan -> ``smo_device``'s dict of another plan on the same resident matrices (the device refit).

    All device work of the device search goes through this function (tests replace it to run the search logic without a GPU)."""
    import torch
    dev = _lib.device_of(device)
    with torch.cuda.device(dev):
        Kd = _gram_device(X, kernels, dev)
        out = smo_device(Kd, plan, dev)
    out["matrix"] = lambda k: Kd[k].cpu().numpy()
    out["solve"] = lambda plan2: smo_device(Kd, plan2, dev)
    return out


def _rows(X):
    """The training rows as a float32 host array, validated on the host with scikit-learn's messages."""
    try:
        import torch
        if isinstance(X, torch.Tensor):
            X = X.detach().cpu().numpy()
    except ImportError:   # pragma: no cover - torch is part of the image
        pass
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("Expected 2D array, got %dD array instead" % X.ndim)
    if X.dtype.kind not in "fiub":
        raise ValueError("GridSearchSVC: rows of dtype %s are not numeric" % X.dtype)
    if X.dtype.kind == "f" and not bool(np.isfinite(X).all()):
        raise ValueError(_NONFINITE)
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    if X.dtype != np.float32 and not np.array_equal(X32.astype(np.float64), X.astype(np.float64)):
        raise ValueError("GridSearchSVC: the rows are taken as float32 (as every entry point of this library takes them), and these "
                         "%s rows are not exactly float32-representable: pass X.astype(np.float32) to search on what the GPU "
                         "computes" % X.dtype)
    return X32


def _sklearn_gamma(gamma, X64):
    """``SVC._gamma`` as ``SVC.fit`` computes it (sklearn/svm/_base.py)."""
    if isinstance(gamma, str):
        if gamma == "scale":
            var = X64.var()
            return 1.0 / (X64.shape[1] * var) if var != 0 else 1.0
        if gamma == "auto":
            return 1.0 / X64.shape[1]
        raise ValueError("gamma %r" % gamma)
    return gamma


def _masked_params(candidates):
    """``param_*`` entries of ``cv_results_`` (GridSearchCV's layout: one masked array per parameter)."""
    vals = {}
    for i, p in enumerate(candidates):
        for name, v in p.items():
            vals.setdefault("param_%s" % name, {})[i] = v
    out = {}
    for key, d in vals.items():
        arr = np.array(list(d.values()))
        dtype = arr.dtype if arr.dtype.kind != "U" and arr.ndim == 1 else object
        ma = np.ma.MaskedArray(np.empty(len(candidates), dtype=dtype), mask=True)
        for i, v in d.items():
            ma[i] = v
        out[key] = ma
    return out


# ---- SVC.fit as one batch of duals: libsvm's svm_train with its Platt cross-validation (sk: = sklearn/svm/src/libsvm/svm.cpp) ----
_FIT_CARRY = ("C", "class_weight", "tol", "shrinking", "max_iter", "probability", "random_state")
_PLATT_FOLDS = 5


def _libsvm_seed(random_state):
    """The seed ``SVC.fit`` hands to libsvm (sklearn/svm/_base.py); ``None`` draws one from NumPy's global state, as there."""
    from sklearn.utils import check_random_state
    return int(check_random_state(random_state).randint(np.iinfo("i").max))


def libsvm_shuffle(seed, l):
    """``rml_libsvm_shuffle``: the permutation of 0 .. l-1 that svm_binary_svc_probability draws (sk:2117-2122) from the seed."""
    perm = np.empty(int(l), dtype=np.int32)
    _lib.check(_lib.load().rml_libsvm_shuffle(int(seed), int(l), perm.ctypes.data), "rml_libsvm_shuffle")
    return perm


def platt_fit(dec, y):
    """``rml_platt_fit``: libsvm's sigmoid_train (sk:1919-2030) on decision values ``dec`` and labels ``y`` (+1 / -1).
    Returns (A, B, info); info 0, or 1 / 2 where libsvm prints "line search fails" / "reaching maximal iterations"."""
    import ctypes
    dec = np.ascontiguousarray(dec, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if dec.ndim != 1 or dec.shape != y.shape:
        raise ValueError("platt_fit: dec and y are 1-D arrays of one length")
    A, B, info = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.check(_lib.load().rml_platt_fit(dec.ctypes.data, y.ctypes.data, len(dec), ctypes.byref(A), ctypes.byref(B), ctypes.byref(info)),
               "rml_platt_fit")
    return A.value, B.value, info.value


def _fit_plan(yi, nc, wC, seed, probability, shrinking, max_iter, tol, matrix=0):
    """The batch of ONE ``SVC.fit`` for ``smo_device``, beside ``GridSearchSVC._smo_plan``: for class indices ``yi`` (0 .. nc-1), the
    per-class weighted C ``wC`` and libsvm's seed, problems 0 .. P-1 are the P = nc(nc-1)/2 pairwise duals of svm_train (rows in
    class order, Cp / Cn as ``_smo_plan`` forms them).  With ``probability`` up to 5 P sub-duals of svm_binary_svc_probability
    (sk:2107-2203) follow: the pair's rows shuffled (``libsvm_shuffle``; the generator is re-seeded for every pair, sk:2373-2376),
    fold f holding out perm[f l / 5 : (f+1) l / 5], each sub-dual in the order libsvm's inner svm_train gives it -- its
    svm_group_classes sorts the labels (sk:2278-2295), so the -1 rows come first (the solver's y = +1 group, with C = Cn), each
    group in shuffle order -- and one SMO_FIT of two classes per fold with held-out rows.  A fold whose training part misses a class
    has no dual (sk:2161-2169: its held-out values are +1 / -1 / 0, kept in ``const_dec``); an empty fold (l < 5) is solved as libsvm
    solves it (it can only set fit_status_) and scored by nothing.
    Returns (plan, meta); meta: per pair ``rows`` (Gram rows, class a then b), ``n_a``, ``const_dec``, and ``held``: (pair, positions
    in the pair's rows, offset into the batch's held-out rows) per fit."""
    pairs = [(a, b) for a in range(nc) for b in range(a + 1, nc)]
    cls_rows = [np.nonzero(yi == c)[0].astype(np.int32) for c in range(nc)]
    problems, rows, fits, test_rows, held = [], [], [], [], []
    n_rows = n_test = 0

    def add(rr, n_pos, Cp, Cn):
        nonlocal n_rows
        problems.append((matrix, len(rr), n_pos, int(bool(shrinking)), int(max_iter), 0, n_rows, n_rows, Cp, Cn, float(tol)))
        rows.append(rr)
        n_rows += len(rr)

    pair_rows = [np.concatenate([cls_rows[a], cls_rows[b]]) for a, b in pairs]
    for (a, b), rr in zip(pairs, pair_rows):
        add(rr, len(cls_rows[a]), wC[a], wC[b])
    const_dec = []
    for p, ((a, b), rr) in enumerate(zip(pairs, pair_rows)):
        if not probability:
            break
        l = len(rr)
        pos = np.arange(l) < len(cls_rows[a])               # y = +1: class a
        perm = libsvm_shuffle(seed, l)
        dec0 = np.zeros(l)
        for f in range(_PLATT_FOLDS):
            b0, e0 = f * l // _PLATT_FOLDS, (f + 1) * l // _PLATT_FOLDS
            tr, te = np.concatenate([perm[:b0], perm[e0:]]), perm[b0:e0]
            n_p = int(pos[tr].sum())
            n_n = len(tr) - n_p
            if n_p == 0 or n_n == 0:
                dec0[te] = 0.0 if n_p == n_n else (1.0 if n_p > 0 else -1.0)
                continue
            # the sub-model's label[0] is -1: its first group is the -1 rows with C = 1 * Cn, then the +1 rows with C = 1 * Cp
            add(rr[np.concatenate([tr[~pos[tr]], tr[pos[tr]]])], n_n, 1.0 * wC[b], 1.0 * wC[a])
            if len(te):
                fits.append((len(problems) - 1, len(te), n_test))
                test_rows.append(rr[te])
                held.append((p, te, n_test))
                n_test += len(te)
        const_dec.append(dec0)
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    plan = {"problems": np.array(problems, dtype=SMO_PROBLEM), "rows": cat(rows), "fits": np.array(fits, dtype=SMO_FIT),
            "test_rows": cat(test_rows), "test_y": np.zeros(n_test, np.int32), "n_classes": 2}
    meta = {"pairs": pairs, "cls_rows": cls_rows, "rows": pair_rows, "const_dec": const_dec, "held": held}
    return plan, meta


def _fit_batch(params, y, run, matrix=0):
    """libsvm's ``SVC(kernel='precomputed', **params).fit(K, y)`` from ONE batch of duals: ``run(plan)`` is ``smo_device`` on the
    matrix K (``_smo`` or its ``solve`` hook).  Every dual of the fit -- the P pairwise ones and, with ``probability``, the sub-duals
    of the Platt cross-validation -- is solved side by side in one ``rml_smo_solve`` call, the held-out rows are scored in one
    ``rml_smo_score`` call, and only alpha, rho, n_iter, stopped and the held-out decision values come back; ``rml_platt_fit`` then
    runs once per pair.  Returns the fitted attributes of that estimator (what ``vars()`` adds to the constructor parameters),
    in libsvm's model layout and with scikit-learn's sign flip of two-class models, without calling libsvm."""
    import warnings
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.utils.class_weight import compute_class_weight
    y = np.asarray(y)
    classes, yi = np.unique(y, return_inverse=True)
    nc = len(classes)
    if not 2 <= nc <= 8:
        raise ValueError("the device SVC fit takes 2..8 classes, got %d" % nc)
    if not float(params["C"]) > 0:
        raise ValueError("C must be > 0, got %r" % (params["C"],))
    class_weight_ = compute_class_weight(params["class_weight"], classes=classes, y=y)
    wC = [float(params["C"]) * float(w) for w in class_weight_]            # libsvm's weighted_C (sk:2455-2468)
    seed = _libsvm_seed(params["random_state"])
    probability = bool(params["probability"])
    plan, meta = _fit_plan(yi.astype(np.int32), nc, wC, seed, probability, params["shrinking"], params["max_iter"], params["tol"], matrix)
    out = run(plan)
    pairs, cls_rows = meta["pairs"], meta["cls_rows"]
    P = len(pairs)
    probs = plan["problems"]
    alphas = [out["alpha"][int(r["alpha_off"]):int(r["alpha_off"]) + int(r["l"])] for r in probs[:P]]

    # svm_train's model (sk:2517-2627): support vectors grouped by class in row order, sv_coef[j-1] / sv_coef[i] of pair (i, j)
    nonzero = np.zeros(len(y), dtype=bool)
    for rr, al in zip(meta["rows"], alphas):
        nonzero[rr[al > 0]] = True
    keep = [nonzero[r] for r in cls_rows]
    n_support = np.array([int(k.sum()) for k in keep], dtype=np.int32)
    support = np.concatenate([r[k] for r, k in zip(cls_rows, keep)]).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(n_support)])
    dual_coef = np.empty((nc - 1, int(n_support.sum())), dtype=np.float64)
    for (a, b), al in zip(pairs, alphas):
        n_a = len(cls_rows[a])
        dual_coef[b - 1, start[a]:start[a + 1]] = al[:n_a][keep[a]]           # alpha * y, y = +1
        dual_coef[a, start[b]:start[b + 1]] = -al[n_a:][keep[b]]              # y = -1
    rho = np.asarray(out["rho"][:P], dtype=np.float64)
    intercept = np.where(rho != 0, -rho, 0.0)                                 # copy_intercept: -rho, never -0.0

    probA, probB = np.empty(0, dtype=np.float64), np.empty(0, dtype=np.float64)
    if probability:
        dec = [d.copy() for d in meta["const_dec"]]
        for p, te, off in meta["held"]:
            dec[p][te] = -out["dec"][off:off + len(te), 0]                    # times submodel->label[0] = -1 (sk:2191)
        probA, probB = np.empty(P, dtype=np.float64), np.empty(P, dtype=np.float64)
        for p, (a, b) in enumerate(pairs):
            yy = np.where(np.arange(len(dec[p])) < len(cls_rows[a]), 1.0, -1.0)
            probA[p], probB[p], _ = platt_fit(dec[p], yy)

    fitted = {"_sparse": False, "class_weight_": class_weight_, "classes_": classes, "_gamma": 0.0, "support_": support,
              "support_vectors_": np.empty((0, 0), dtype=np.float64), "_n_support": n_support, "dual_coef_": dual_coef,
              "intercept_": intercept, "_probA": probA, "_probB": probB, "fit_status_": int(bool((out["stopped"] == 1).any())),
              "_num_iter": np.asarray(out["n_iter"][:P], dtype=np.int32).copy(), "shape_fit_": (len(y), len(y)),
              "n_features_in_": len(y)}
    if fitted["fit_status_"] == 1:
        warnings.warn("Solver terminated early (max_iter=%i).  Consider pre-processing your data with StandardScaler or MinMaxScaler."
                      % params["max_iter"], ConvergenceWarning)
    # SVC.fit after libsvm returns (sklearn/svm/_base.py): the internal copies, then the sign flip of two-class models
    fitted["_intercept_"] = intercept.copy()
    fitted["_dual_coef_"] = dual_coef
    if nc == 2:
        fitted["intercept_"] = intercept * -1
        fitted["dual_coef_"] = -dual_coef
    if not (np.isfinite(fitted["_intercept_"]).all() and np.isfinite(dual_coef).all()):
        raise ValueError("The dual coefficients or intercepts are not finite. The input data may contain large values and need to be "
                         "preprocessed.")
    fitted["n_iter_"] = fitted["_num_iter"]
    return fitted


def _adopt(est, fitted, X32, key):
    """Turn the ``linear`` / ``rbf`` estimator ``est`` into the fitted one from the fitted attributes of its precomputed-kernel twin
    on the rows ``X32``: the support vectors are the training rows, shape and gamma are those of a fit on the rows."""
    X64 = X32.astype(np.float64)
    vars(est).update(fitted)
    est.support_vectors_ = X64[est.support_]
    est.shape_fit_ = X32.shape
    est.n_features_in_ = X32.shape[1]
    est._gamma = _sklearn_gamma(est.gamma, X64) if key[0] == "linear" else est.gamma
    return est


def _check_kernel(who, kernel, gamma, C):
    if kernel not in ("linear", "rbf"):
        raise NotImplementedError("%s: kernel %r (the HIP Gram pass computes 'linear' and 'rbf')" % (who, kernel))
    if kernel == "rbf":
        if isinstance(gamma, str):
            raise NotImplementedError("%s: gamma=%r depends on each fold's rows; give numeric gammas" % (who, gamma))
        if not np.isfinite(float(gamma)) or float(gamma) < 0:
            raise ValueError("%s: gamma must be a finite non-negative number, got %r" % (who, gamma))
    if not float(C) > 0:
        raise ValueError("%s: C must be > 0, got %r" % (who, C))


def fit_svc(estimator, X, y, device=None):
    """``estimator.fit(X, y)`` for an unfitted ``sklearn.svm.SVC`` with kernel ``linear`` or ``rbf`` (numeric gamma), on the GPU: the
    kernel matrix by ``rml_gram``, every dual of libsvm's fit in one ``rml_smo_solve`` call (its 5-fold Platt cross-validation
    included when ``probability=True``), libsvm's sigmoid fit by ``rml_platt_fit``.  ``C``, ``class_weight``, ``tol``, ``shrinking``,
    ``max_iter``, ``probability`` and ``random_state`` are honoured (``random_state=None`` draws a seed as scikit-learn does);
    ``sample_weight`` is not supported.  On the same kernel matrix the result is what libsvm computes, bit for bit.  Returns the
    estimator, fitted: a genuine ``SVC`` that predicts, pickles and converts (``from_sklearn``) like any other."""
    from sklearn.svm import SVC
    if type(estimator) is not SVC:
        raise NotImplementedError("fit_svc fits sklearn.svm.SVC, not %s" % type(estimator).__name__)
    params = estimator.get_params()
    _check_kernel("fit_svc", params["kernel"], params["gamma"], params["C"])
    X32 = _rows(X)
    y = np.asarray(y)
    if y.ndim != 1 or y.shape[0] != X32.shape[0]:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (X32.shape[0], len(y)))
    key = ("linear", None) if params["kernel"] == "linear" else ("rbf", float(params["gamma"]))
    fitted = _fit_batch({k: params[k] for k in _FIT_CARRY}, y, lambda plan: _smo(X32, [key], plan, device))
    return _adopt(estimator, fitted, X32, key)


class GridSearchSVC:
    """``GridSearchCV(SVC(...), param_grid)`` for C, ``linear`` / ``rbf`` kernels and numeric gamma, on GPU kernel matrices.

    The subset of ``GridSearchCV``'s surface that train.py uses: ``fit(X, y)``, ``best_estimator_``, ``best_params_``, ``best_score_``,
    ``best_index_``, ``cv_results_``, ``n_splits_``, ``refit_time_``, ``scorer_`` (accuracy).  Fit order: rows validated; every distinct
    kernel of the grid computed by ``rml_gram`` (grouped so that the host copies stay under ``max_gram_bytes``); the candidates in
    ``ParameterGrid`` order x the splits fitted by libsvm on ``K[train, train]`` and scored on ``K[test, train]`` on a pool of
    ``n_jobs`` threads (libsvm releases the GIL); the best point refitted on all rows.

    ``solver="device"`` keeps the kernel matrices on the GPU and replaces the host fits and scores of the search: per group of
    kernels, every candidate x split x class-pair dual is solved by ONE ``rml_smo_solve`` call (libsvm's SMO, one workgroup per
    dual, the same iterates bit for bit) and every held-out row is scored by ONE ``rml_smo_score`` call; only the winner's matrix
    is copied back, for the same host refit (``probability`` and libsvm's Platt step included).  ``tol``, ``shrinking``,
    ``max_iter`` and ``class_weight`` of the base estimator are honoured (weighted C as scikit-learn forms it: ``compute_class_weight``
    on the fold's labels, times C).  A split whose training rows miss a class is fitted on the host as before.  The batch has no
    per-fit times: ``fit_time`` / ``score_time`` of a device fit are the batch's solve / score time divided evenly among its fits.
    ``solver="host"`` (the default) is the search described above.

    ``refit_solver="device"`` refits the winner on the GPU as well (``fit_svc``'s batch: the duals of libsvm's fit and of its Platt
    cross-validation in one ``rml_smo_solve`` call, ``rml_platt_fit`` per class pair) -- after a device search on the matrix still
    resident there, so that no kernel matrix is copied back at all.  The estimator is the same, bit for bit.
    ``refit_solver="host"`` (the default) is libsvm's fit on the host copy of the winner's matrix."""

    def __init__(self, estimator, param_grid, cv=5, n_jobs=4, refit=True, device=None, max_gram_bytes=8 << 30, scoring=None,
                 verbose=0, solver="host", refit_solver="host"):
        self.estimator = estimator
        self.param_grid = param_grid
        self.cv = cv
        self.n_jobs = n_jobs
        self.refit = refit
        self.device = device
        self.max_gram_bytes = max_gram_bytes
        self.scoring = scoring
        self.verbose = verbose
        self.solver = solver
        self.refit_solver = refit_solver

    # ---- argument checks (before any work) ----
    def _check(self):
        from sklearn.model_selection import ParameterGrid
        from sklearn.svm import SVC
        if self.solver not in ("host", "device"):
            raise ValueError("GridSearchSVC: solver must be 'host' or 'device', got %r" % (self.solver,))
        if self.refit_solver not in ("host", "device"):
            raise ValueError("GridSearchSVC: refit_solver must be 'host' or 'device', got %r" % (self.refit_solver,))
        if type(self.estimator) is not SVC:
            raise NotImplementedError("GridSearchSVC searches sklearn.svm.SVC, not %s" % type(self.estimator).__name__)
        if self.scoring not in (None, "accuracy"):
            raise NotImplementedError("GridSearchSVC scores by accuracy (SVC.score, GridSearchCV's default), not %r" % (self.scoring,))
        if callable(self.refit) or not isinstance(self.refit, bool):
            raise NotImplementedError("GridSearchSVC: refit must be True or False, not %r" % (self.refit,))
        grids = [self.param_grid] if isinstance(self.param_grid, dict) else list(self.param_grid)
        for g in grids:
            bad = sorted(set(g) - set(_GRID_KEYS))
            if bad:
                raise NotImplementedError("GridSearchSVC searches %s, not %s" % (", ".join(_GRID_KEYS), ", ".join(bad)))
        candidates = list(ParameterGrid(self.param_grid))
        base = self.estimator.get_params()
        for p in candidates:
            kernel = p.get("kernel", base["kernel"])
            gamma = p.get("gamma", base["gamma"])
            if kernel not in ("linear", "rbf"):
                raise NotImplementedError("GridSearchSVC: kernel %r (the HIP Gram pass computes 'linear' and 'rbf')" % (kernel,))
            if kernel == "rbf":
                if isinstance(gamma, str):
                    raise NotImplementedError("GridSearchSVC: gamma=%r depends on each fold's rows; give numeric gammas" % gamma)
                if not np.isfinite(float(gamma)) or float(gamma) < 0:
                    raise ValueError("GridSearchSVC: gamma must be a finite non-negative number, got %r" % (gamma,))
            if not float(p.get("C", base["C"])) > 0:
                raise ValueError("GridSearchSVC: C must be > 0, got %r" % (p.get("C", base["C"]),))
        return candidates, base

    def _key(self, p, base):
        kernel = p.get("kernel", base["kernel"])
        return ("linear", None) if kernel == "linear" else ("rbf", float(p.get("gamma", base["gamma"])))

    def _svc(self, p, base, kernel, probability=None):
        from sklearn.svm import SVC
        kw = {k: base[k] for k in _CARRY}
        kw["C"] = p.get("C", base["C"])
        if probability is not None:
            kw["probability"] = probability
        return SVC(kernel=kernel, **kw)

    def _smo_plan(self, candidates, base, grp, splits, y):
        """The batch of one group of kernels for ``_smo``: per candidate of the group (ParameterGrid order) and split, one fit made of
        one dual per class pair in libsvm's order.  Returns (plan, [(ci, si) of fit f], [(ci, si) left to the host])."""
        from sklearn.utils.class_weight import compute_class_weight
        classes = np.unique(y)
        nc = len(classes)
        yi = np.searchsorted(classes, y).astype(np.int32)
        pairs = [(a, b) for a in range(nc) for b in range(a + 1, nc)]
        rows, test_rows, test_y = [], [], []
        per_split = {}                      # si -> ([(rows_off, l, n_pos) per pair], class weights)
        n_rows = 0
        for si, (tr, te) in enumerate(splits):
            if not 2 <= nc <= 8 or len(np.unique(yi[tr])) < nc or len(te) == 0:
                continue                    # a class without rows in this fold: libsvm fits another model -- the host path's job
            cw = base["class_weight"]
            w = np.ones(nc) if cw is None else compute_class_weight(cw, classes=classes, y=y[tr])
            subs = []
            for a, b in pairs:
                ra, rb = tr[yi[tr] == a], tr[yi[tr] == b]
                rows += [ra, rb]
                subs.append((n_rows, len(ra) + len(rb), len(ra)))
                n_rows += len(ra) + len(rb)
            per_split[si] = (subs, w)
        problems, fits, on_device, host = [], [], [], []
        n_alpha = n_test = 0
        for ci, p in enumerate(candidates):
            key = self._key(p, base)
            if key not in grp:
                continue
            C = float(p.get("C", base["C"]))
            for si, (tr, te) in enumerate(splits):
                if si not in per_split:
                    host.append((ci, si))
                    continue
                subs, w = per_split[si]
                fits.append((len(problems), len(te), n_test))
                on_device.append((ci, si))
                test_rows.append(te)
                test_y.append(yi[te])
                n_test += len(te)
                for (off, l, n_pos), (a, b) in zip(subs, pairs):
                    problems.append((grp.index(key), l, n_pos, int(bool(base["shrinking"])), int(base["max_iter"]), 0, off, n_alpha,
                                     C * w[a], C * w[b], float(base["tol"])))
                    n_alpha += l
        cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
        plan = {"problems": np.array(problems, dtype=SMO_PROBLEM), "rows": cat(rows), "fits": np.array(fits, dtype=SMO_FIT),
                "test_rows": cat(test_rows), "test_y": cat(test_y), "n_classes": nc}
        return plan, on_device, host

    def fit(self, X, y):
        from sklearn.base import clone
        from sklearn.metrics import accuracy_score, make_scorer
        from sklearn.model_selection import check_cv
        candidates, base = self._check()
        X32 = _rows(X)
        y = np.asarray(y)
        if y.ndim != 1 or y.shape[0] != X32.shape[0]:
            raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (X32.shape[0], len(y)))
        N, D = X32.shape
        cv = check_cv(self.cv, y, classifier=True)
        splits = [(np.asarray(tr), np.asarray(te)) for tr, te in cv.split(X32, y)]
        n_splits = len(splits)
        if n_splits == 0:
            raise ValueError("No fits were performed. Was the CV iterator empty? Were there no candidates?")
        if not candidates:
            raise ValueError("No fits were performed. Was the CV iterator empty? Were there no candidates?")

        keys = []
        for p in candidates:
            k = self._key(p, base)
            if k not in keys:
                keys.append(k)
        mat_bytes = N * N * 8
        per = min(8, int(self.max_gram_bytes // mat_bytes))
        if per < 1:
            raise ValueError("GridSearchSVC: one %d x %d kernel matrix takes %d bytes, more than max_gram_bytes=%d"
                             % (N, N, mat_bytes, self.max_gram_bytes))
        groups = [keys[i:i + per] for i in range(0, len(keys), per)]
        # joblib's convention (what GridSearchCV's n_jobs means): None -> 1, -1 -> every CPU this process may use, -2 -> all but one;
        # joblib counts the CPUs of the process's affinity mask and cgroup quota, not the whole machine's
        from joblib import effective_n_jobs
        nj = max(1, min(effective_n_jobs(self.n_jobs), len(candidates) * n_splits))
        if self.verbose > 0:
            print("Fitting %d folds for each of %d candidates, totalling %d fits" % (n_splits, len(candidates),
                                                                                   n_splits * len(candidates)), flush=True)

        scores = np.zeros((len(candidates), n_splits))
        fit_t = np.zeros_like(scores)
        score_t = np.zeros_like(scores)

        # The split fits run WITHOUT libsvm's Platt step (probability=False), whatever the base estimator says: the score is
        # accuracy of predict(), which does not use the Platt parameters, and the SMO solve is the same either way (libsvm fits
        # the pairwise models independently of the Platt cross-validation), so decision values and split scores are the bits
        # GridSearchCV gets -- at a sixth of the SMO work.  It also keeps libsvm's process-wide random generator (used only by
        # that cross-validation, outside the GIL) out of the concurrent fits.  The refit below keeps the base estimator's setting.
        def one(K, ci, si):
            tr, te = splits[si]
            est = self._svc(candidates[ci], base, "precomputed", probability=False)
            t0 = time.perf_counter()
            est.fit(K[np.ix_(tr, tr)], y[tr])
            t1 = time.perf_counter()
            s = est.score(K[np.ix_(te, tr)], y[te])
            t2 = time.perf_counter()
            scores[ci, si], fit_t[ci, si], score_t[ci, si] = s, t1 - t0, t2 - t1
            if self.verbose > 1:
                p = candidates[ci]
                print("[CV %d/%d] END %s; total time=%5.1fs" % (si + 1, n_splits, ", ".join("%s=%s" % (k, p[k]) for k in sorted(p)),
                                                             t2 - t0), flush=True)

        mats = {}
        fetch = {}                              # device search: kernel key -> function returning its host matrix (last group only)
        resident = {}                           # device search: kernel key -> (matrix index, solve hook) of the resident matrices (same)
        with ThreadPoolExecutor(max_workers=nj) as pool:
            for grp in groups:
                todo = [(ci, si) for ci, p in enumerate(candidates) if self._key(p, base) in grp for si in range(n_splits)]
                if self.solver == "device":
                    plan, on_device, todo = self._smo_plan(candidates, base, grp, splits, y)
                    out = _smo(X32, grp, plan, self.device)
                    fetch = {k: (lambda i=i, m=out["matrix"]: m(i)) for i, k in enumerate(grp)}
                    resident = {k: (i, out["solve"]) for i, k in enumerate(grp)} if "solve" in out else {}
                    mats = {}
                    for f, (ci, si) in enumerate(on_device):
                        scores[ci, si] = float(out["correct"][f]) / len(splits[si][1])
                        fit_t[ci, si] = out["solve_s"] / len(on_device)
                        score_t[ci, si] = out["score_s"] / len(on_device)
                        if self.verbose > 1:
                            p = candidates[ci]
                            print("[CV %d/%d] END %s; total time=%5.1fs" % (si + 1, n_splits, ", ".join("%s=%s" % (k, p[k]) for k in sorted(p)),
                                                                         fit_t[ci, si] + score_t[ci, si]), flush=True)
                    for k in sorted({self._key(candidates[ci], base) for ci, _ in todo}, key=grp.index):
                        mats[k] = fetch[k]()
                else:
                    mats = dict(zip(grp, _gram(X32, grp, self.device)))
                jobs = [pool.submit(one, mats[self._key(candidates[ci], base)], ci, si) for ci, si in todo]
                for j in jobs:
                    j.result()

        res = {}

        def store(name, arr, splits_=False, rank=False):
            if splits_:
                for s in range(n_splits):
                    res["split%d_%s" % (s, name)] = arr[:, s]
            mean = np.average(arr, axis=1)
            res["mean_%s" % name] = mean
            res["std_%s" % name] = np.sqrt(np.average((arr - mean[:, None]) ** 2, axis=1))
            if rank:
                from scipy.stats import rankdata
                res["rank_%s" % name] = rankdata(-mean, method="min").astype(np.int32, copy=False)

        store("fit_time", fit_t)
        store("score_time", score_t)
        res.update(_masked_params(candidates))
        res["params"] = candidates
        store("test_score", scores, splits_=True, rank=True)
        self.cv_results_ = res
        self.n_splits_ = n_splits
        self.scorer_ = make_scorer(accuracy_score)
        self.multimetric_ = False
        self.best_index_ = int(res["rank_test_score"].argmin())
        self.best_score_ = float(res["mean_test_score"][self.best_index_])
        self.best_params_ = candidates[self.best_index_]

        if self.refit:
            best = self.best_params_
            key = self._key(best, base)
            if self.refit_solver == "device":
                # the winner's matrix where the search left it, or (host search, or a winner of an earlier group) computed again
                matrix, run = resident.get(key, (0, lambda plan: _smo(X32, [key], plan, self.device)))
                params = {k: base[k] for k in _FIT_CARRY}
                params["C"] = best.get("C", base["C"])
                t0 = time.perf_counter()
                fitted = _fit_batch(params, y, run, matrix)
                self.refit_time_ = time.perf_counter() - t0
            else:
                K = mats[key] if key in mats else fetch[key]() if key in fetch else _gram(X32, [key], self.device)[0]
                t0 = time.perf_counter()
                pre = self._svc(best, base, "precomputed").fit(K, y)
                self.refit_time_ = time.perf_counter() - t0
                params = pre.get_params()
                fitted = {k: v for k, v in vars(pre).items() if k not in params}
            self.best_estimator_ = _adopt(clone(self.estimator).set_params(**best), fitted, X32, key)
        self.classes_ = np.unique(y)
        return self

    # GridSearchCV delegates these to best_estimator_
    def predict(self, X):
        return self.best_estimator_.predict(X)

    def decision_function(self, X):
        return self.best_estimator_.decision_function(X)

    def predict_proba(self, X):
        return self.best_estimator_.predict_proba(X)

    def score(self, X, y):
        return self.best_estimator_.score(X, y)


def find_best_svm_estimator(X, y, cv, random_seed, solver="host", refit_solver="host"):
    """Exhaustive search over specified parameter values for svm (train.py:462-491, the same grid, base estimator and log lines).
    ``solver="device"`` runs the search's fits on the GPU and ``refit_solver="device"`` the refit of the winner (GridSearchSVC);
    the result is the same.

    Returns:
        optimized svm estimator.

    Note:
        https://www.csie.ntu.edu.tw/~cjlin/papers/guide/guide.pdf
    """
    from sklearn import svm
    print('\n Finding best svm estimator...')
    Cs = [0.01, 0.1, 1, 10, 100]
    gammas = [0.001, 0.01, 0.1, 1, 10]
    param_grid = [
        {'C': Cs, 'kernel': ['linear']},
        {'C': Cs, 'gamma': gammas, 'kernel': ['rbf']}
    ]
    init_est = svm.SVC(probability=True, class_weight='balanced',
                       random_state=random_seed, cache_size=1000, verbose=False)
    grid_search = GridSearchSVC(estimator=init_est, param_grid=param_grid, verbose=2, n_jobs=4, cv=cv, solver=solver,
                                refit_solver=refit_solver)
    grid_search.fit(X, y)
    logger.info('\n Best estimator:')
    logger.info(grid_search.best_estimator_)
    logger.info('\n Best score for {}-fold search:'.format(grid_search.n_splits_))
    logger.info(grid_search.best_score_)
    logger.info('\n Best hyperparameters:')
    logger.info(grid_search.best_params_)
    return grid_search.best_estimator_
