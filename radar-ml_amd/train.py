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


def _gram(X, kernels, device=None):
    """Every kernel matrix of ``kernels`` (a list of ('linear', None) / ('rbf', gamma), at most 8) of the float32 rows ``X`` against
    themselves: one upload, one ``rml_gram`` call, one copy back.  Returns a list of host (N, N) float64 matrices.

    All device work of the search goes through this function (tests replace it to run the search logic without a GPU)."""
    import torch
    lib = _lib.load()
    if not 1 <= len(kernels) <= 8:
        raise ValueError("_gram: 1..8 kernels per call, got %d" % len(kernels))
    N, D = X.shape
    dev = _lib.device_of(device)
    ctx = _lib.context(dev)
    kinds = np.array([_lib.GRAM_LINEAR if k == "linear" else _lib.GRAM_RBF for k, _ in kernels], dtype=np.int32)
    gammas = np.array([0.0 if g is None else float(g) for _, g in kernels], dtype=np.float64)
    with torch.cuda.device(dev):
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        out = torch.empty((len(kernels), N, N), dtype=torch.float64, device=dev)
        _lib.check(lib.rml_gram(ctx, _lib.ptr(Xd), D, N, D, len(kernels), kinds.ctypes.data, gammas.ctypes.data, _lib.ptr(out),
                                N, N * N, _lib.stream_ptr(dev)), "rml_gram")
        host = out.cpu().numpy()
    return [host[k] for k in range(len(kernels))]


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


class GridSearchSVC:
    """``GridSearchCV(SVC(...), param_grid)`` for C, ``linear`` / ``rbf`` kernels and numeric gamma, on GPU kernel matrices.

    The subset of ``GridSearchCV``'s surface that train.py uses: ``fit(X, y)``, ``best_estimator_``, ``best_params_``, ``best_score_``,
    ``best_index_``, ``cv_results_``, ``n_splits_``, ``refit_time_``, ``scorer_`` (accuracy).  Fit order: rows validated; every distinct
    kernel of the grid computed by ``rml_gram`` (grouped so that the host copies stay under ``max_gram_bytes``); the candidates in
    ``ParameterGrid`` order x the splits fitted by libsvm on ``K[train, train]`` and scored on ``K[test, train]`` on a pool of
    ``n_jobs`` threads (libsvm releases the GIL); the best point refitted on all rows."""

    def __init__(self, estimator, param_grid, cv=5, n_jobs=4, refit=True, device=None, max_gram_bytes=8 << 30, scoring=None,
                 verbose=0):
        self.estimator = estimator
        self.param_grid = param_grid
        self.cv = cv
        self.n_jobs = n_jobs
        self.refit = refit
        self.device = device
        self.max_gram_bytes = max_gram_bytes
        self.scoring = scoring
        self.verbose = verbose

    # ---- argument checks (before any work) ----
    def _check(self):
        from sklearn.model_selection import ParameterGrid
        from sklearn.svm import SVC
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
        with ThreadPoolExecutor(max_workers=nj) as pool:
            for grp in groups:
                mats = dict(zip(grp, _gram(X32, grp, self.device)))
                jobs = [pool.submit(one, mats[self._key(p, base)], ci, si)
                        for ci, p in enumerate(candidates) if self._key(p, base) in mats for si in range(n_splits)]
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
            K = mats[key] if key in mats else _gram(X32, [key], self.device)[0]
            t0 = time.perf_counter()
            pre = self._svc(best, base, "precomputed").fit(K, y)
            self.refit_time_ = time.perf_counter() - t0
            est = clone(self.estimator).set_params(**best)
            X64 = X32.astype(np.float64)
            params = pre.get_params()
            fitted = {k: v for k, v in vars(pre).items() if k not in params}
            vars(est).update(fitted)
            est.support_vectors_ = X64[pre.support_]
            est.shape_fit_ = (N, D)
            est.n_features_in_ = D
            est._gamma = _sklearn_gamma(est.gamma, X64) if key[0] == "linear" else est.gamma
            self.best_estimator_ = est
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


def find_best_svm_estimator(X, y, cv, random_seed):
    """Exhaustive search over specified parameter values for svm (train.py:462-491, the same grid, base estimator and log lines).

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
    grid_search = GridSearchSVC(estimator=init_est, param_grid=param_grid, verbose=2, n_jobs=4, cv=cv)
    grid_search.fit(X, y)
    logger.info('\n Best estimator:')
    logger.info(grid_search.best_estimator_)
    logger.info('\n Best score for {}-fold search:'.format(grid_search.n_splits_))
    logger.info(grid_search.best_score_)
    logger.info('\n Best hyperparameters:')
    logger.info(grid_search.best_params_)
    return grid_search.best_estimator_
