"""The training side of the reference's ``train.py`` on the GPU: its SVC and SGD fits, their grid searches, its online loop.

Every estimator that leaves this module is a genuine scikit-learn one (``SVC``, ``SGDClassifier``, ``CalibratedClassifierCV``), so
what the reference does with it afterwards (the pickle, predict.py, ``from_sklearn``) works unchanged.  In file order:

* Device hooks: ``_gram`` (``rml_gram``: every kernel matrix of a grid from one upload), ``_smo`` (``smo_device``: libsvm's duals and
  their held-out scores, batched, on matrices that stay on the device), their twins for the projection-mask search ``_gram_masks`` /
  ``_smo_masks`` (``rml_gram_segments`` once, ``rml_gram_compose`` per group of mask x kernel matrices), ``_sgd`` (``sgd_device``: scikit-learn's SGD problems, batched)
  and ``_sgd_online`` (``sgd_online_device``: a chain of partial_fit steps in one call).  All device work of the rest of the module
  goes through these six names, looked up in the module at call time (tests replace them with NumPy twins).
* Fits: ``fit_svc`` (``SVC.fit``, Platt step included), ``fit_sgd`` / ``partial_fit_sgd`` and the chain ``partial_fit_sgd_steps``.
* Searches: ``GridSearchSVC`` (and ``ProjMaskSearchSVC``, which adds the projection mask to its candidates) and ``GridSearchSGD``
  on one ``GridSearchCV`` scaffold, inside the reference's ``find_best_*``.
* Flows: ``sgd_fit`` / ``svc_fit`` (``svc_fit_masks``: the mask chosen by the search) of the reference (features, ``balance_classes``, augment epochs, search or online chain).
* Calibration and evaluation: ``calibrate_prefit`` and ``evaluate_model``.
"""
import logging
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

RANDOM_SEED = 1234                      # train.py:32
_NONFINITE = "Input contains NaN, infinity or a value too large for dtype('float64')."      # scikit-learn's message


def _cat_i32(parts):
    return np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)


# ---- device hooks: the Gram pass and libsvm's duals on it (rml_gram, rml_smo_solve / rml_smo_score) --------------------------------
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


# ---- device hooks of the projection-mask search: per-segment inner products once, mask x kernel matrices composed from them --------
# A mask key is (bits, 'linear', None) / (bits, 'rbf', gamma): bit s selects segment s of the rows (common._mask_bits' order).
_segment_cache = {}                     # the resident products of ONE set of rows (ProjMaskSearchSVC.fit releases them)


def _release_segments():
    _segment_cache.clear()


def segment_products_device(Xd, segments, device=None):
    """``rml_gram_segments`` on the DEVICE rows ``Xd`` ((N, sum(segments)) float32): the DEVICE tensors ``G`` (nseg, N, N) and ``nsq``
    (nseg, N), float64, of the inner products and squared row norms of every segment (all lengths positive)."""
    import torch
    lib = _lib.load()
    dev, ctx, N, D, ld = _device_rows("segment_products_device", Xd, device)
    seg = np.array([int(v) for v in segments], dtype=np.int64)
    if len(seg) < 1 or (seg < 1).any() or int(seg.sum()) != D:
        raise ValueError("segment_products_device: %r are not positive lengths that add up to the %d columns" % (list(segments), D))
    with torch.cuda.device(dev):
        G = torch.empty((len(seg), N, N), dtype=torch.float64, device=dev)
        nsq = torch.empty((len(seg), N), dtype=torch.float64, device=dev)
        _lib.check(lib.rml_gram_segments(ctx, _lib.ptr(Xd), ld, N, len(seg), seg.ctypes.data, _lib.ptr(G), N, N * N, _lib.ptr(nsq),
                                         _lib.stream_ptr(dev)), "rml_gram_segments")
    return G, nsq


def compose_device(G, nsq, keys, device=None):
    """``rml_gram_compose``: the kernel matrices of the mask keys ``keys`` (bits over the segments of ``G`` / ``nsq``, as
    ``segment_products_device`` returns them) as a DEVICE (len(keys), N, N) float64 tensor, each bit-exactly symmetric."""
    import torch
    lib = _lib.load()
    dev = _lib.device_of(device if device is not None else G.device)
    nseg, N = int(G.shape[0]), int(G.shape[1])
    bits = np.array([b for b, _, _ in keys], dtype=np.int32)
    kinds = np.array([_lib.GRAM_LINEAR if k == "linear" else _lib.GRAM_RBF for _, k, _ in keys], dtype=np.int32)
    gammas = np.array([0.0 if g is None else float(g) for _, _, g in keys], dtype=np.float64)
    with torch.cuda.device(dev):
        out = torch.empty((len(keys), N, N), dtype=torch.float64, device=dev)
        _lib.check(lib.rml_gram_compose(_lib.context(dev), _lib.ptr(G), N, N * N, _lib.ptr(nsq), N, nseg, len(keys), bits.ctypes.data,
                                        kinds.ctypes.data, gammas.ctypes.data, _lib.ptr(out), N, N * N, _lib.stream_ptr(dev)),
                   "rml_gram_compose")
    return out


def _mask_matrices_device(X, segments, keys, dev):
    """The DEVICE (len(keys), N, N) matrices of the mask keys of the float32 host rows ``X``: the rows uploaded and their segment
    products formed on the first call for these rows, and kept resident for the following ones."""
    import torch
    segments = tuple(int(v) for v in segments)
    used = [i for i, n in enumerate(segments) if n > 0]          # rml_gram_segments takes positive lengths
    tag = (id(X), X.shape, segments, str(dev))
    entry = _segment_cache.get("entry")
    if entry is None or entry[0] != tag:
        _release_segments()
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        entry = (tag, X) + segment_products_device(Xd, [segments[i] for i in used], dev)     # X: keeps id(X) from being reused
        _segment_cache["entry"] = entry
    dense = []
    for bits, kernel, gamma in keys:
        if bits < 1 or bits >> len(segments) or any(bits >> i & 1 and segments[i] == 0 for i in range(len(segments))):
            raise ValueError("mask bits %d select no segment or an empty one of %r" % (bits, segments))
        dense.append((sum(1 << j for j, i in enumerate(used) if bits >> i & 1), kernel, gamma))
    return compose_device(entry[2], entry[3], dense, dev)


def _gram_masks(X, segments, keys, device=None):
    """Every kernel matrix of the mask keys ``keys`` of the float32 rows ``X`` (full rows: the concatenation of ``segments``
    columns each): one upload and one ``rml_gram_segments`` pass per set of rows, one ``rml_gram_compose`` call, one copy back.
    Returns a list of host (N, N) float64 matrices.

    All device work of the host mask search goes through this function (tests replace it to run the search logic without a GPU)."""
    import torch
    dev = _lib.device_of(device)
    with torch.cuda.device(dev):
        host = _mask_matrices_device(X, segments, keys, dev).cpu().numpy()
    return [host[k] for k in range(len(keys))]


def _smo_masks(X, segments, keys, plan, device=None):
    """``_smo`` for mask keys: the matrices composed from the resident segment products stay ON THE DEVICE, every dual of ``plan``
    is solved and every held-out row scored there (``smo_device``).  Returns ``smo_device``'s dict plus ``matrix`` and ``solve``.

    All device work of the device mask search goes through this function (tests replace it to run the search logic without a GPU)."""
    import torch
    dev = _lib.device_of(device)
    with torch.cuda.device(dev):
        Kd = _mask_matrices_device(X, segments, keys, dev)
        out = smo_device(Kd, plan, dev)
    out["matrix"] = lambda k: Kd[k].cpu().numpy()
    out["solve"] = lambda plan2: smo_device(Kd, plan2, dev)
    return out


# ---- device hooks: scikit-learn's SGD problems, batched (rml_sgd_solve / rml_sgd_score) --------------------------------------------
# rml_sgd_problem / rml_sgd_fit of include/radarml.h
SGD_PROBLEM = np.dtype([("n", "<i4"), ("penalty", "<i4"), ("average", "<i4"), ("max_iter", "<i4"), ("n_iter_no_change", "<i4"),
                        ("shuffle", "<i4"), ("seed", "<u4"), ("warm", "<i4"), ("rows_off", "<i8"), ("y_off", "<i8"), ("out", "<i8"),
                        ("alpha", "<f8"), ("l1_ratio", "<f8"), ("tol", "<f8"), ("weight_pos", "<f8"), ("weight_neg", "<f8"), ("t0", "<f8")])
SGD_FIT = np.dtype([("prob0", "<i4"), ("n_test", "<i4"), ("test_off", "<i8")])
_SGD_PENALTY = {"l1": _lib.SGD_L1, "l2": _lib.SGD_L2, "elasticnet": _lib.SGD_ELASTICNET}


def sgd_shuffle(seed, perm):
    """``rml_sgd_shuffle``: one ``SequentialDataset.shuffle(seed)`` pass (Fisher-Yates on scikit-learn's xorshift generator) over the
    int32 index array ``perm``; returns the permuted copy."""
    perm = np.array(perm, dtype=np.int32)
    _lib.check(_lib.load().rml_sgd_shuffle(int(seed), len(perm), perm.ctypes.data), "rml_sgd_shuffle")
    return perm


def _device_rows(who, Xd, device):
    """(dev, ctx, N, D, ld) for the C calls of ``who`` on the DEVICE rows ``Xd``; ld is the row stride."""
    import torch
    dev = _lib.device_of(device if device is not None else Xd.device)
    ctx = _lib.context(dev)
    if Xd.dtype != torch.float32 or Xd.dim() != 2 or Xd.stride(1) != 1 or Xd.stride(0) < Xd.shape[1]:
        raise ValueError("%s: the rows are an (N, D) float32 tensor with unit column stride" % who)
    return dev, ctx, int(Xd.shape[0]), int(Xd.shape[1]), int(Xd.stride(0))


def sgd_device(Xd, plan, device=None, check=True):
    """``rml_sgd_solve`` + ``rml_sgd_score`` on the DEVICE rows ``Xd`` (an (N, D) float32 tensor with unit column stride; its row
    stride is the ld of the C call) for ``plan``: a dict of
    ``problems`` (SGD_PROBLEM records), ``rows`` / ``y`` (int32: the problems' rows and 0 / 1 labels), ``n_out`` (output slots),
    ``fits`` (SGD_FIT records), ``test_rows`` / ``test_y`` (int32: held-out rows and their class indices), ``n_classes`` and, for
    warm problems, ``init``: host arrays ``coef`` / ``avg_coef`` (n_out, D) and ``intercept`` / ``avg_intercept`` (n_out).
    Returns host arrays ``intercept``, ``avg_intercept``, ``n_iter``, ``t``, ``status`` per slot, ``dec``, ``labels`` per held-out
    row, ``correct`` per fit, ``solve_s`` / ``score_s`` (the wall time of the two batched calls), and ``coefs``: a function
    slots -> host (coef, avg_coef) of those slots (the weights stay on the device until asked for).  A problem or a held-out row
    that names a row outside the matrix raises RadarMLError (``check=False``: status -1 / label -1 are returned instead)."""
    import torch
    lib = _lib.load()
    dev, ctx, N, D, ld = _device_rows("sgd_device", Xd, device)
    probs = np.ascontiguousarray(plan["problems"], dtype=SGD_PROBLEM)
    fits = np.ascontiguousarray(plan.get("fits", np.zeros(0, SGD_FIT)), dtype=SGD_FIT)
    n_out = int(plan["n_out"])
    C = int(plan.get("n_classes", 2))
    n_dec = 1 if C == 2 else C
    with torch.cuda.device(dev):
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        rows, y = i32(plan["rows"]), i32(plan["y"])
        te_rows, te_y = i32(plan.get("test_rows", np.zeros(0, np.int32))), i32(plan.get("test_y", np.zeros(0, np.int32)))
        n_test = int(te_rows.numel())
        init = plan.get("init")
        f64 = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(shape)).to(dev)
        if init is None:
            coef = torch.zeros((max(n_out, 1), D), dtype=torch.float64, device=dev)
            avg_coef = torch.zeros_like(coef)
            icpt = torch.zeros(max(n_out, 1), dtype=torch.float64, device=dev)
            avg_icpt = torch.zeros_like(icpt)
        else:
            coef, avg_coef = f64(init["coef"], (n_out, D)), f64(init["avg_coef"], (n_out, D))
            icpt, avg_icpt = f64(init["intercept"], (n_out,)), f64(init["avg_intercept"], (n_out,))
        n_iter = torch.zeros(max(n_out, 1), dtype=torch.int32, device=dev)
        t = torch.zeros(max(n_out, 1), dtype=torch.float64, device=dev)
        status = torch.zeros(max(n_out, 1), dtype=torch.int32, device=dev)
        dec = torch.zeros(max(n_test * n_dec, 1), dtype=torch.float64, device=dev)
        labels = torch.zeros(max(n_test, 1), dtype=torch.int32, device=dev)
        correct = torch.zeros(max(len(fits), 1), dtype=torch.int32, device=dev)
        st = _lib.stream_ptr(dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        _lib.check(lib.rml_sgd_solve(ctx, _lib.ptr(Xd), N, D, ld, probs.ctypes.data, len(probs), _lib.ptr(rows), int(rows.numel()),
                                     _lib.ptr(y), int(y.numel()), n_out, _lib.ptr(coef), _lib.ptr(avg_coef), _lib.ptr(icpt),
                                     _lib.ptr(avg_icpt), _lib.ptr(n_iter), _lib.ptr(t), _lib.ptr(status), st), "rml_sgd_solve")
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if len(fits):
            _lib.check(lib.rml_sgd_score(ctx, _lib.ptr(Xd), N, D, ld, probs.ctypes.data, len(probs), n_out, _lib.ptr(coef),
                                         _lib.ptr(avg_coef), _lib.ptr(icpt), _lib.ptr(avg_icpt), _lib.ptr(t), C, fits.ctypes.data,
                                         len(fits), _lib.ptr(te_rows), _lib.ptr(te_y), n_test, _lib.ptr(dec), _lib.ptr(labels),
                                         _lib.ptr(correct), st), "rml_sgd_score")
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()

        def coefs(slots):
            with torch.cuda.device(dev):
                idx = torch.as_tensor(list(slots), dtype=torch.long, device=dev)
                return coef[idx].cpu().numpy(), avg_coef[idx].cpu().numpy()

        out = {"intercept": icpt.cpu().numpy()[:n_out], "avg_intercept": avg_icpt.cpu().numpy()[:n_out],
               "n_iter": n_iter.cpu().numpy()[:n_out], "t": t.cpu().numpy()[:n_out], "status": status.cpu().numpy()[:n_out],
               "dec": dec.cpu().numpy()[:n_test * n_dec].reshape(n_test, n_dec), "labels": labels.cpu().numpy()[:n_test],
               "correct": correct.cpu().numpy()[:len(fits)], "solve_s": t1 - t0, "score_s": t2 - t1, "coefs": coefs}
    if check and (out["status"][probs["out"]] < 0).any():
        raise _lib.RadarMLError("rml_sgd_solve: a problem names a row outside the matrix")
    if check and (out["labels"] < 0).any():
        raise _lib.RadarMLError("rml_sgd_score: a held-out row outside the matrix")
    return out


def _sgd(X, plan, device=None):
    """The float32 host rows ``X`` uploaded ONCE, every problem of ``plan`` solved on them in one ``rml_sgd_solve`` call and every
    held-out row scored in one ``rml_sgd_score`` call (``sgd_device``).  Returns ``sgd_device``'s dict plus ``solve``: a function
    plan -> ``sgd_device``'s dict of another plan on the same resident rows (the refit of a search's winner).

    All device work of the SGD fits and of their search goes through this function (tests replace it to run the logic without a GPU)."""
    import torch
    dev = _lib.device_of(device)
    with torch.cuda.device(dev):
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        out = sgd_device(Xd, plan, dev)
    out["solve"] = lambda plan2: sgd_device(Xd, plan2, dev)
    return out


# ---- device hooks: a chain of partial_fit calls resident on the device (rml_sgd_online) --------------------------------------------
# rml_sgd_step of include/radarml.h
SGD_STEP = np.dtype([("off", "<i8"), ("n", "<i4"), ("score", "<i4"), ("seed", "<u4", (8,))])


def sgd_online_device(Xd, plan, device=None, check=True, fill=None):
    """``rml_sgd_online`` on the DEVICE rows ``Xd`` (as ``sgd_device`` takes them) for ``plan``: a dict of ``problems`` (K SGD_PROBLEM
    records of one estimator, class order; K = 1 for two classes), ``n_classes``, ``steps`` (SGD_STEP records), ``rows`` / ``cls``
    (int32: the steps' rows and their class indices), ``test_rows`` / ``test_y`` (int32, optional), ``init`` (host ``coef`` /
    ``avg_coef`` (K, D), ``intercept`` / ``avg_intercept`` (K): the state of problem k, stored at its slot), ``avg_flag`` and
    optionally ``n_out`` (output slots, default K).  Returns host arrays per PROBLEM ``coef``, ``avg_coef``, ``intercept``,
    ``avg_intercept``, ``t``, ``status``, and ``avg_flag``, ``fail_step``, ``correct`` (per step), ``labels`` / ``dec`` (of the last
    scored step).  Two uploads, one call, two copies back: the only wait is for those.  A row outside the matrix raises
    RadarMLError (``check=False``: status -1 is returned).  ``fill``: what the outputs without an initial value hold before the
    call (default 0)."""
    import torch
    lib = _lib.load()
    dev, ctx, N, D, ld = _device_rows("sgd_online_device", Xd, device)
    probs = np.ascontiguousarray(plan["problems"], dtype=SGD_PROBLEM)
    steps = np.ascontiguousarray(plan["steps"], dtype=SGD_STEP)
    C = int(plan["n_classes"])
    K, n_dec, S = len(probs), (1 if C == 2 else C), len(steps)
    if K != n_dec:
        raise ValueError("sgd_online_device: %d problems for %d classes" % (K, C))
    n_out = int(plan.get("n_out", K))
    out = probs["out"].astype(np.int64)
    if ((out < 0) | (out >= n_out)).any():
        raise ValueError("sgd_online_device: an output slot outside [0, %d)" % n_out)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ravel()
    rows, cls = i32(plan["rows"]), i32(plan["cls"])
    te_rows, te_y = i32(plan.get("test_rows", [])), i32(plan.get("test_y", []))
    n_test = len(te_rows)
    init = plan["init"]
    fill = 0 if fill is None else fill
    # one float64 and one int32 block hold every in / out array: [coef | avg_coef | intercept | avg_intercept | t | dec] and
    # [status | avg_flag | fail_step | correct | labels | rows | cls | test_rows | test_y]
    f_off = np.cumsum([0, n_out * D, n_out * D, n_out, n_out, n_out, max(n_test * n_dec, 1)])
    hf = np.full(int(f_off[-1]), float(fill))
    for name, j, width in (("coef", 0, D), ("avg_coef", 1, D), ("intercept", 2, 1), ("avg_intercept", 3, 1)):
        hf[f_off[j]:f_off[j + 1]].reshape(n_out, width)[out] = np.asarray(init[name], dtype=np.float64).reshape(K, width)
    i_off = np.cumsum([0, n_out, 1, 1, max(S, 1), max(n_test, 1), max(len(rows), 1), max(len(cls), 1), max(n_test, 1), max(n_test, 1)])
    hi = np.full(int(i_off[-1]), int(fill), dtype=np.int32)
    hi[i_off[1]] = int(bool(plan.get("avg_flag", False)))
    for j, a in ((5, rows), (6, cls), (7, te_rows), (8, te_y)):
        hi[i_off[j]:i_off[j] + len(a)] = a
    with torch.cuda.device(dev):
        df, di = torch.from_numpy(hf).to(dev), torch.from_numpy(hi).to(dev)
        fp = lambda j: _lib.ptr(df[int(f_off[j]):])
        ip = lambda j: _lib.ptr(di[int(i_off[j]):])
        _lib.check(lib.rml_sgd_online(ctx, _lib.ptr(Xd), N, D, ld, probs.ctypes.data, C, steps.ctypes.data, S, ip(5), ip(6), len(rows),
                                      ip(7), ip(8), n_test, n_out, fp(0), fp(1), fp(2), fp(3), fp(4), ip(1), ip(0), ip(2), ip(3), ip(4), fp(5),
                                      _lib.stream_ptr(dev)), "rml_sgd_online")
        rf, ri = df.cpu().numpy(), di[:int(i_off[5])].cpu().numpy()
    f = lambda j, width: rf[f_off[j]:f_off[j + 1]].reshape(n_out, width)[out]
    res = {"coef": f(0, D), "avg_coef": f(1, D), "intercept": f(2, 1)[:, 0], "avg_intercept": f(3, 1)[:, 0], "t": f(4, 1)[:, 0],
           "status": ri[:n_out][out], "avg_flag": bool(ri[i_off[1]]), "fail_step": int(ri[i_off[2]]), "correct": ri[i_off[3]:i_off[3] + S],
           "labels": ri[i_off[4]:i_off[4] + n_test], "dec": rf[f_off[5]:f_off[5] + n_test * n_dec].reshape(n_test, n_dec)}
    if check and (res["status"] < 0).any():
        raise _lib.RadarMLError("rml_sgd_online: a step or the held-out list names a row outside the matrix")
    return res


def _sgd_online(X, plan, device=None):
    """The rows ``X`` (float32 host rows, uploaded ONCE, or a CUDA tensor taken where it is) and the whole chain of partial_fit steps
    of ``plan`` in one ``rml_sgd_online`` call (``sgd_online_device``).

    All device work of ``partial_fit_sgd_steps`` goes through this function (tests replace it to run the logic without a GPU)."""
    import torch
    dev = _lib.device_of(device if device is not None or not isinstance(X, torch.Tensor) else X.device)
    with torch.cuda.device(dev):
        Xd = X.to(dev) if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        return sgd_online_device(Xd, plan, dev)


# ---- argument checks shared by the fits and the searches (before any device work) -------------------------------------------------
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


def _check_y(X32, y):
    y = np.asarray(y)
    if y.ndim != 1 or y.shape[0] != X32.shape[0]:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (X32.shape[0], len(y)))
    return y


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


def _kernel_key(kernel, gamma):
    """The kernel of a checked (kernel, gamma) as ``_gram`` / ``_smo`` name it."""
    return ("linear", None) if kernel == "linear" else ("rbf", float(gamma))


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
    plan = {"problems": np.array(problems, dtype=SMO_PROBLEM), "rows": _cat_i32(rows), "fits": np.array(fits, dtype=SMO_FIT),
            "test_rows": _cat_i32(test_rows), "test_y": np.zeros(n_test, np.int32), "n_classes": 2}
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
    y = _check_y(X32, y)
    key = _kernel_key(params["kernel"], params["gamma"])
    fitted = _fit_batch({k: params[k] for k in _FIT_CARRY}, y, lambda plan: _smo(X32, [key], plan, device))
    return _adopt(estimator, fitted, X32, key)


# ---- SGDClassifier(loss='log_loss').fit / partial_fit (sk: = sklearn/linear_model/_stochastic_gradient.py, scikit-learn 1.7.2) -----
_SGD_OVERFLOW = "Floating-point under-/overflow occurred at epoch #%d. Scaling input data with StandardScaler or MinMaxScaler might help."
_SGD_MAX_ITER = ("Maximum number of iteration reached before convergence. Consider increasing max_iter to improve the fit.")


def _sgd_seeds(random_state, n_classes):
    """The shuffle seed of each binary problem of one ``SGDClassifier.fit`` / ``partial_fit``, drawn as scikit-learn draws them: for
    more than two classes _fit_multiclass draws one seed per class (sk:784-785) and fit_binary makes a generator from each; for two
    classes fit_binary takes ``random_state`` itself (sk:736-751).  From that generator the first draw seeds the dataset
    (make_dataset; unused by the solver) and the second is the shuffle seed (sk:460)."""
    from sklearn.utils import check_random_state
    max_int = np.iinfo(np.int32).max
    if n_classes == 2:
        states = [check_random_state(random_state)]
    else:
        states = [check_random_state(s) for s in check_random_state(random_state).randint(max_int, size=n_classes)]
    seeds = []
    for rs in states:
        rs.randint(1, max_int)
        seeds.append(int(rs.randint(max_int)))
    return seeds


def _sgd_params(params, who):
    """The solver's view of SGDClassifier parameters; raises for what the device fit does not do, before any device work."""
    loss = params["loss"]
    if loss not in ("log_loss", "log"):
        raise NotImplementedError("%s: loss=%r (the device fit is logistic regression, loss='log_loss')" % (who, loss))
    if params["learning_rate"] != "optimal":
        raise NotImplementedError("%s: learning_rate=%r (the device fit runs the 'optimal' schedule)" % (who, params["learning_rate"]))
    if params["early_stopping"]:
        raise NotImplementedError("%s: early_stopping=True" % who)
    if not params["fit_intercept"]:
        raise NotImplementedError("%s: fit_intercept=False" % who)
    if params["penalty"] not in _SGD_PENALTY:
        raise NotImplementedError("%s: penalty=%r (l2, l1 or elasticnet)" % (who, params["penalty"]))
    alpha = float(params["alpha"])
    if not (alpha > 0 and np.isfinite(alpha)):
        raise ValueError("alpha must be > 0 since learning_rate is 'optimal'. alpha is used to compute the optimal learning rate.")
    l1_ratio = 0.15 if params["l1_ratio"] is None else float(params["l1_ratio"])
    if not 0 <= l1_ratio <= 1:
        raise ValueError("l1_ratio must be in [0, 1], got %r" % (params["l1_ratio"],))
    average = params["average"]
    average = int(average) if isinstance(average, (bool, np.bool_)) or float(average) == int(average) else -1
    if average < 0:
        raise ValueError("average must be a bool or a non-negative integer, got %r" % (params["average"],))
    max_iter, n_nc = int(params["max_iter"]), int(params["n_iter_no_change"])
    if max_iter < 1 or n_nc < 1:
        raise ValueError("max_iter and n_iter_no_change must be >= 1, got %r and %r" % (params["max_iter"], params["n_iter_no_change"]))
    tol = params["tol"]
    return {"penalty": _SGD_PENALTY[params["penalty"]], "alpha": alpha, "l1_ratio": l1_ratio, "average": average, "max_iter": max_iter,
            "tol": -np.inf if tol is None else float(tol), "n_iter_no_change": n_nc, "shuffle": int(bool(params["shuffle"]))}


def _sgd_problem(prm, n, seed, rows_off, y_off, out, weight_pos, weight_neg, t0=1.0, warm=0, max_iter=None):
    return (n, prm["penalty"], prm["average"], prm["max_iter"] if max_iter is None else max_iter, prm["n_iter_no_change"], prm["shuffle"],
            seed, warm, rows_off, y_off, out, prm["alpha"], prm["l1_ratio"], prm["tol"], weight_pos, weight_neg, t0)


def _sgd_check_rows(who, n):
    if n > _lib.SGD_MAX_ROWS:
        raise NotImplementedError("%s: %d training rows (rml_sgd_solve takes at most %d per problem)" % (who, n, _lib.SGD_MAX_ROWS))


def _sgd_check_overflow(out):
    if (out["status"] == 2).any():
        raise ValueError(_SGD_OVERFLOW % int(out["n_iter"][np.nonzero(out["status"] == 2)[0][0]]))


class _SGDState:
    """The solver's side of an ``SGDClassifier`` (``prm``: its ``_sgd_params``) whose ``classes_``, parameter arrays, ``t_`` and
    ``_expanded_class_weight`` are in place, as fit_binary and _prepare_fit_binary (sk:348-365, 736-751) see it: one problem per class
    of ``positives`` (the second class alone for two), each on views of the estimator's arrays, so that what they alias stays aliased."""

    def __init__(self, est, prm):
        self.est, self.prm, self.nc = est, prm, len(est.classes_)
        self.positives = [1] if self.nc == 2 else list(range(self.nc))
        self.avg = prm["average"] > 0

    def views(self, c):
        """(coef, intercept, avg_coef, avg_intercept, j) of class ``c``: its weight rows, and the intercept arrays with its index."""
        est, K = self.est, len(self.positives)
        j = 0 if self.nc == 2 else c
        if self.avg:
            return est._standard_coef.reshape(K, -1)[j], est._standard_intercept, est._average_coef.reshape(K, -1)[j], est._average_intercept, j
        return est.coef_.reshape(K, -1)[j], est.intercept_, None, None, j

    def init(self):
        """The state of every problem as the ``init`` of a plan: host ``coef`` / ``avg_coef`` (K, D), ``intercept`` / ``avg_intercept`` (K)."""
        K, D = len(self.positives), self.est.coef_.shape[-1]
        init = {"coef": np.zeros((K, D)), "avg_coef": np.zeros((K, D)), "intercept": np.zeros(K), "avg_intercept": np.zeros(K)}
        for k, c in enumerate(self.positives):
            coef, icpt, acoef, aicpt, j = self.views(c)
            init["coef"][k], init["intercept"][k] = coef, icpt[j]
            if self.avg:
                init["avg_coef"][k], init["avg_intercept"][k] = acoef, aicpt[j]
        return init

    def problems(self, n, seeds, y_offs, max_iter):
        """The warm SGD_PROBLEM records from ``t_`` on: problem k on ``n`` rows, its labels at ``y_offs[k]``, to output slot k."""
        w = self.est._expanded_class_weight
        return np.array([_sgd_problem(self.prm, n, seeds[k], 0, y_offs[k], k, w[c], w[0] if self.nc == 2 else 1.0, t0=float(self.est.t_),
                                      warm=1, max_iter=max_iter) for k, c in enumerate(self.positives)], dtype=SGD_PROBLEM)

    def store(self, coefs, avg_coefs, avg_intercept):
        """Write the solver's weights (per problem) back through the views; the standard intercept is the caller's."""
        for k, c in enumerate(self.positives):
            coef, _, acoef, aicpt, j = self.views(c)
            coef[:] = coefs[k]
            if self.avg:
                acoef[:] = avg_coefs[k]
                aicpt[j] = avg_intercept[k]

    def select(self, averaged):
        """With averaging on: ``coef_`` / ``intercept_`` alias the averaged or the standard arrays, as scikit-learn leaves them."""
        est = self.est
        coef = est._average_coef if averaged else est._standard_coef
        est.coef_ = coef.reshape(1, -1) if self.nc == 2 else coef
        est.intercept_ = est._average_intercept if averaged else est._standard_intercept


def _sgd_run(est, y, max_iter, run, who):
    """``BaseSGDClassifier._partial_fit`` (sk:583-666) after its validation, on an estimator whose ``classes_``, parameter arrays and
    ``t_`` are in place: one problem per class (one for two classes) from the estimator's current state, solved by ``run(plan)``
    (``_sgd`` or its ``solve`` hook on rows 0 .. len(y)-1), and the results stored by the statements of fit_binary, _fit_binary and
    _fit_multiclass (sk:497-503, 753-768, 807-823) on the estimator's own arrays, so that what they alias stays aliased."""
    from sklearn.utils.class_weight import compute_class_weight
    prm = _sgd_params(est.get_params(), who)
    classes = est.classes_
    nc, n = len(classes), len(y)
    _sgd_check_rows(who, n)
    yi = np.searchsorted(classes, y)
    if ((yi >= nc) | (classes[np.minimum(yi, nc - 1)] != y)).any():
        raise ValueError("%s: y holds labels outside classes_ %r" % (who, classes))
    est._expanded_class_weight = compute_class_weight(est.class_weight, classes=classes, y=y)
    st = _SGDState(est, prm)
    K = len(st.positives)
    seeds = _sgd_seeds(est.random_state, nc)
    plan = {"problems": st.problems(n, seeds, [k * n for k in range(K)], max_iter), "rows": np.arange(n, dtype=np.int32),
            "y": np.concatenate([(yi == c).astype(np.int32) for c in st.positives]), "n_out": K, "init": st.init(), "n_classes": nc}
    out = run(plan)
    _sgd_check_overflow(out)
    st.store(*out["coefs"](range(K)), out["avg_intercept"])
    n_iter_ = int(out["n_iter"][:K].max())
    # the tail of _fit_binary (sk:753-768) for two classes, of _fit_multiclass (sk:807-823) for more
    if nc == 2:
        intercept = np.atleast_1d(float(out["intercept"][0]))
    else:
        for k in range(K):
            est.intercept_[k] = out["intercept"][k]
        intercept = est.intercept_
    est.t_ += n_iter_ * n
    est.n_iter_ = n_iter_
    if st.avg:
        averaged = prm["average"] <= est.t_ - 1
        if not averaged:
            est._standard_intercept = np.atleast_1d(intercept)
        st.select(averaged)
    elif nc == 2:
        est.coef_ = est.coef_.reshape(1, -1)
        est.intercept_ = intercept
    return est


def _sgd_prepare(est, who):
    """Type and parameter checks of an estimator for the device fit (before any device work); the reference's old spelling
    ``loss='log'`` and its float ``max_iter`` are rewritten to what scikit-learn 1.7 takes."""
    from sklearn.linear_model import SGDClassifier
    if type(est) is not SGDClassifier:
        raise NotImplementedError("%s fits sklearn.linear_model.SGDClassifier, not %s" % (who, type(est).__name__))
    prm = _sgd_params(est.get_params(), who)
    est.set_params(loss="log_loss", max_iter=prm["max_iter"])
    return prm


def _sgd_fit(est, X32, y, run, who):
    """``BaseSGDClassifier._fit`` (sk:668-734) of a prepared estimator on validated rows, the solver run by ``run``."""
    import warnings
    from sklearn.exceptions import ConvergenceWarning
    classes = np.unique(y)
    if not 2 <= len(classes) <= 8:
        raise ValueError("%s takes 2..8 classes, got %d" % (who, len(classes)))
    for name in ("classes_", "_standard_coef", "_standard_intercept", "_average_coef", "_average_intercept"):
        if hasattr(est, name):
            delattr(est, name)
    est.coef_ = est.intercept_ = None
    est.t_ = 1.0
    est.classes_ = classes
    est.n_features_in_ = X32.shape[1]
    est._allocate_parameter_mem(n_classes=len(classes), n_features=X32.shape[1], input_dtype=np.float64)
    est._loss_function_ = est._get_loss_function(est.loss)
    _sgd_run(est, y, est.max_iter, run, who)
    if est.tol is not None and est.tol > -np.inf and est.n_iter_ == est.max_iter:
        warnings.warn(_SGD_MAX_ITER, ConvergenceWarning)
    return est


def fit_sgd(estimator, X, y, device=None):
    """``estimator.fit(X, y)`` for an unfitted ``sklearn.linear_model.SGDClassifier`` on the GPU: one ``rml_sgd_solve`` call, one
    workgroup per class (one for two classes) running scikit-learn's ``_plain_sgd64``.  Supported: ``loss='log_loss'`` (or the old
    spelling ``'log'``), ``learning_rate='optimal'``, ``early_stopping=False``, ``fit_intercept=True``, 2..8 classes; honoured:
    ``penalty``, ``alpha``, ``l1_ratio``, ``average``, ``max_iter`` (through ``int()``), ``tol``, ``n_iter_no_change``, ``shuffle``,
    ``random_state``, ``class_weight``; anything else raises ``NotImplementedError``; ``sample_weight`` and sparse rows are not
    supported.  Apart from the summation order of the dot product the arithmetic is scikit-learn's.  Returns the estimator, fitted:
    a genuine ``SGDClassifier`` that predicts, pickles, calibrates and converts (``from_sklearn``) like any other; it warns
    (``ConvergenceWarning``) and raises (``ValueError`` on overflow) where scikit-learn would."""
    _sgd_prepare(estimator, "fit_sgd")
    X32 = _rows(X)
    y = _check_y(X32, y)
    _sgd_check_rows("fit_sgd", len(y))
    return _sgd_fit(estimator, X32, y, lambda plan: _sgd(X32, plan, device), "fit_sgd")


def partial_fit_sgd(estimator, X, y, classes=None, device=None):
    """``estimator.partial_fit(X, y, classes)`` on the GPU, as train.py:432 calls it: one epoch from the estimator's current state
    (its weights, ``t_`` and the averaged weights carried over).  The estimator and its restrictions are ``fit_sgd``'s."""
    who = "partial_fit_sgd"
    _sgd_prepare(estimator, who)
    X32 = _rows(X)
    y = _check_y(X32, y)
    est = estimator
    _sgd_partial_prepare(est, X32.shape[1], classes, who)
    return _sgd_run(est, y, 1, lambda plan: _sgd(X32, plan, device), who)


# ---- the online loop of train.py:409-438 as one resident chain ---------------------------------------------------------------------
def _sgd_partial_prepare(est, n_features, classes, who):
    """What ``SGDClassifier.partial_fit`` does to the estimator before its solver runs (sk:583-631)."""
    if est.class_weight == "balanced" and not hasattr(est, "classes_"):
        raise ValueError("class_weight 'balanced' is not supported for partial_fit. In order to use 'balanced' weights, use "
                         "compute_class_weight('balanced', classes=classes, y=y).")
    if not hasattr(est, "classes_"):
        if classes is None:
            raise ValueError("classes must be passed on the first call to partial_fit.")
        est.classes_ = np.unique(np.asarray(classes))
        if not 2 <= len(est.classes_) <= 8:
            raise ValueError("%s takes 2..8 classes, got %d" % (who, len(est.classes_)))
        est.n_features_in_ = n_features
    elif classes is not None and not np.array_equal(est.classes_, np.unique(np.asarray(classes))):
        raise ValueError("`classes=%r` is not the same as on last call to partial_fit, was: %r" % (classes, est.classes_))
    if getattr(est, "coef_", None) is None:
        est._allocate_parameter_mem(n_classes=len(est.classes_), n_features=n_features, input_dtype=np.float64)
    elif n_features != est.coef_.shape[-1]:
        raise ValueError("Number of features %d does not match previous data %d." % (n_features, est.coef_.shape[-1]))
    est._loss_function_ = est._get_loss_function(est.loss)
    if not hasattr(est, "t_"):
        est.t_ = 1.0


def partial_fit_sgd_steps(estimator, X, y, steps, classes=None, test=None, score_every=1, device=None):
    """The chain ``for rows in steps: estimator.partial_fit(X[rows], y[rows], classes)`` of train.py:409-416 and 425-438 on the GPU
    as ONE ``rml_sgd_online`` call: the rows go up at most once, the weights never leave the chip between the steps, and the only
    wait is for the results.  ``X``: host rows or a CUDA float32 tensor; ``y``: the labels of all its rows; ``steps``: a sequence of
    row-index arrays (1 .. 8 192 rows each), one partial_fit call each, in the order the call would see its rows.
    ``test=(row indices, labels)``: held-out rows of ``X`` that are predicted after every ``score_every``-th step (the steps
    ``score_every - 1``, ``2 score_every - 1``, ..).  Returns ``(estimator, accuracies)``: the estimator as the chain of
    ``partial_fit_sgd`` calls leaves it (a genuine ``SGDClassifier``: ``t_``, ``n_iter_ == 1``, the four weight arrays, ``coef_`` /
    ``intercept_`` aliased as scikit-learn aliases them) and per step the accuracy on the held-out rows (NaN where the step was
    not scored).  The estimator, its restrictions and its errors are ``partial_fit_sgd``'s; where scikit-learn would raise its
    overflow ``ValueError`` in some step, this raises it after the call and leaves the estimator as it was before the call."""
    from sklearn.utils.class_weight import compute_class_weight
    who = "partial_fit_sgd_steps"
    est = estimator
    _sgd_prepare(est, who)
    try:
        import torch
        on_device = isinstance(X, torch.Tensor) and X.is_cuda
    except ImportError:   # pragma: no cover - torch is part of the image
        on_device = False
    if on_device:
        if X.dim() != 2 or X.dtype != torch.float32:
            raise ValueError("%s: device rows are an (N, D) float32 tensor" % who)
        rows_of = X
    else:
        rows_of = _rows(X)
    y = _check_y(rows_of, y)
    N, D = int(rows_of.shape[0]), int(rows_of.shape[1])
    if est.class_weight == "balanced":
        raise ValueError("class_weight 'balanced' is not supported for partial_fit. In order to use 'balanced' weights, use "
                         "compute_class_weight('balanced', classes=classes, y=y).")
    _sgd_partial_prepare(est, D, classes, who)
    prm = _sgd_params(est.get_params(), who)
    steps = [np.asarray(s, dtype=np.int64).ravel() for s in steps]
    if not steps:
        return est, np.zeros(0)
    for s, rr in enumerate(steps):
        if len(rr) < 1:
            raise ValueError("%s: step %d has no rows" % (who, s))
        _sgd_check_rows(who, len(rr))
        if rr.min() < 0 or rr.max() >= N:
            raise IndexError("%s: step %d names a row outside the %d rows" % (who, s, N))
    classes_ = est.classes_
    nc = len(classes_)

    def class_index(lab, strict):
        idx = np.searchsorted(classes_, lab)
        miss = (idx >= nc) | (classes_[np.minimum(idx, nc - 1)] != lab)
        if strict and miss.any():
            raise ValueError("%s: y holds labels outside classes_ %r" % (who, classes_))
        return np.where(miss, -1, idx).astype(np.int32)

    used = np.unique(np.concatenate(steps))
    yi = np.full(N, -1, dtype=np.int32)
    yi[used] = class_index(y[used], True)
    est._expanded_class_weight = compute_class_weight(est.class_weight, classes=classes_, y=y[steps[-1]])
    st = _SGDState(est, prm)
    K = len(st.positives)
    score_every = int(score_every)
    if score_every < 1:
        raise ValueError("%s: score_every must be >= 1" % who)
    if test is not None:
        te_rows = np.asarray(test[0], dtype=np.int64).ravel()
        te_y = class_index(np.asarray(test[1]).ravel(), False)
        if len(te_rows) != len(te_y) or len(te_rows) < 1:
            raise ValueError("%s: test is (row indices, labels) of equal, non-zero length" % who)
    else:
        te_rows, te_y = np.zeros(0, np.int64), np.zeros(0, np.int32)
    # the shuffle seeds, drawn per call as scikit-learn draws them (the same every call for an integer random_state)
    fixed = _sgd_seeds(est.random_state, nc) if isinstance(est.random_state, (int, np.integer)) else None
    rec = np.zeros(len(steps), dtype=SGD_STEP)
    off, offs = 0, {}
    row_parts = []
    for s, rr in enumerate(steps):
        key = rr.tobytes()
        if key not in offs:                     # identical steps (the online_learn chain) share one range of the list
            offs[key] = off
            row_parts.append(rr)
            off += len(rr)
        rec[s]["off"], rec[s]["n"] = offs[key], len(rr)
        rec[s]["score"] = int(test is not None and (s + 1) % score_every == 0)
        rec[s]["seed"][:K] = fixed if fixed is not None else _sgd_seeds(est.random_state, nc)
    rows = np.concatenate(row_parts)
    # the rows, labels and seeds of a problem are its steps': the records carry the estimator's state and parameters
    plan = {"problems": st.problems(1, [0] * K, [0] * K, 1), "n_classes": nc, "steps": rec, "rows": rows.astype(np.int32),
            "cls": yi[rows], "test_rows": te_rows.astype(np.int32), "test_y": te_y, "init": st.init(),
            "avg_flag": bool(st.avg and est.intercept_ is est._average_intercept)}
    out = _sgd_online(rows_of, plan, device)
    if (out["status"] == 2).any():
        raise ValueError(_SGD_OVERFLOW % 1)
    st.store(out["coef"], out["avg_coef"], out["avg_intercept"])
    SI = np.array(out["intercept"], dtype=np.float64)
    est.t_ = float(out["t"].max())
    est.n_iter_ = 1
    if st.avg:
        # the standard intercept in an array of its own, as _fit_binary / _fit_multiclass leave it once averaging has begun
        if est._standard_intercept is est._average_intercept:
            est._standard_intercept = SI
        else:
            est._standard_intercept[:] = SI
        st.select(out["avg_flag"])
    else:
        est.coef_ = est.coef_.reshape(K, -1)
        if nc == 2:
            est.intercept_ = np.atleast_1d(SI[0])
        else:
            est.intercept_[:] = SI
    acc = np.full(len(steps), np.nan)
    scored = out["correct"] >= 0
    if len(te_rows):
        acc[scored] = out["correct"][scored].astype(np.float64) / len(te_rows)
    return est, acc


# ---- the searches: GridSearchCV's scaffold, GridSearchSVC, GridSearchSGD ------------------------------------------------------------
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


def _cv_results(candidates, n_splits, fit_t, score_t, scores):
    """``cv_results_`` in GridSearchCV's layout from (candidate, split) arrays of fit times, score times and test scores."""
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
    return res


class _GridSearch:
    """What ``GridSearchSVC`` and ``GridSearchSGD`` share of ``GridSearchCV``'s scaffold; a subclass has its plan builder and ``fit``."""

    def __init__(self, estimator, param_grid, cv, n_jobs, refit, device, scoring, verbose):
        self.estimator = estimator
        self.param_grid = param_grid
        self.cv = cv
        self.n_jobs = n_jobs
        self.refit = refit
        self.device = device
        self.scoring = scoring
        self.verbose = verbose

    def _check_search(self, who, est_type, accuracy_of, grid_keys):
        """The checks of the search ``who`` for estimators of exactly ``est_type`` over ``grid_keys`` (``accuracy_of``: a word on its
        score).  Returns (candidates in ``ParameterGrid`` order, the base estimator's parameters)."""
        from sklearn.model_selection import ParameterGrid
        if type(self.estimator) is not est_type:        # named by its public module: sklearn.svm._classes -> sklearn.svm
            raise NotImplementedError("%s searches %s.%s, not %s" % (who, est_type.__module__.split("._")[0], est_type.__name__,
                                                                    type(self.estimator).__name__))
        if self.scoring not in (None, "accuracy"):
            raise NotImplementedError("%s scores by accuracy (%s), not %r" % (who, accuracy_of, self.scoring))
        if callable(self.refit) or not isinstance(self.refit, bool):
            raise NotImplementedError("%s: refit must be True or False, not %r" % (who, self.refit))
        grids = [self.param_grid] if isinstance(self.param_grid, dict) else list(self.param_grid)
        for g in grids:
            bad = sorted(set(g) - set(grid_keys))
            if bad:
                raise NotImplementedError("%s searches %s, not %s" % (who, ", ".join(grid_keys), ", ".join(bad)))
        return list(ParameterGrid(self.param_grid)), self.estimator.get_params()

    def _check_data(self, X32, y):
        """What a subclass asks of the validated rows and labels (raises)."""

    def _setup(self, X, y, candidates):
        """The validated float32 rows, the labels and the list of (train, test) splits; prints the header of the search."""
        from sklearn.model_selection import check_cv
        X32 = _rows(X)
        y = _check_y(X32, y)
        self._check_data(X32, y)
        cv = check_cv(self.cv, y, classifier=True)
        splits = [(np.asarray(tr), np.asarray(te)) for tr, te in cv.split(X32, y)]
        if not splits or not candidates:
            raise ValueError("No fits were performed. Was the CV iterator empty? Were there no candidates?")
        if self.verbose > 0:
            print("Fitting %d folds for each of %d candidates, totalling %d fits" % (len(splits), len(candidates),
                                                                                   len(splits) * len(candidates)), flush=True)
        return X32, y, splits

    def _end_line(self, p, si, n_splits, seconds):
        """The line of one finished fit: candidate ``p`` on split ``si``."""
        if self.verbose > 1:
            print("[CV %d/%d] END %s; total time=%5.1fs" % (si + 1, n_splits, ", ".join("%s=%s" % (k, p[k]) for k in sorted(p)), seconds),
                  flush=True)

    def _finish(self, candidates, n_splits, fit_t, score_t, scores):
        """``cv_results_`` .. ``best_params_`` from the (candidate, split) arrays of fit times, score times and test scores."""
        from sklearn.metrics import accuracy_score, make_scorer
        res = _cv_results(candidates, n_splits, fit_t, score_t, scores)
        self.cv_results_ = res
        self.n_splits_ = n_splits
        self.scorer_ = make_scorer(accuracy_score)
        self.multimetric_ = False
        self.best_index_ = int(res["rank_test_score"].argmin())
        self.best_score_ = float(res["mean_test_score"][self.best_index_])
        self.best_params_ = candidates[self.best_index_]

    # GridSearchCV delegates these to best_estimator_
    def predict(self, X):
        return self.best_estimator_.predict(X)

    def decision_function(self, X):
        return self.best_estimator_.decision_function(X)

    def predict_proba(self, X):
        return self.best_estimator_.predict_proba(X)

    def score(self, X, y):
        return self.best_estimator_.score(X, y)


def _log_best(grid_search):
    """The lines the reference's ``find_best_*`` log after their search; returns the winner."""
    logger.info('\n Best estimator:')
    logger.info(grid_search.best_estimator_)
    logger.info('\n Best score for {}-fold search:'.format(grid_search.n_splits_))
    logger.info(grid_search.best_score_)
    logger.info('\n Best hyperparameters:')
    logger.info(grid_search.best_params_)
    return grid_search.best_estimator_


# ---- GridSearchSVC and the reference's find_best_svm_estimator ---------------------------------------------------------------------
_GRID_KEYS = ("C", "kernel", "gamma")
# SVC constructor parameters that carry from the base estimator into every fit
_CARRY = ("C", "probability", "class_weight", "random_state", "cache_size", "tol", "shrinking", "max_iter",
          "decision_function_shape", "break_ties")
# where the kernel matrices of a searched group are afterwards, three dicts by kernel key: ``host`` copies, ``fetch`` functions that
# copy one back from the device, ``resident`` (matrix index, ``solve`` hook) pairs of those kept there
_Matrices =namedtuple("_Matrices", "host fetch resident")


class GridSearchSVC(_GridSearch):
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
        super().__init__(estimator, param_grid, cv, n_jobs, refit, device, scoring, verbose)
        self.max_gram_bytes = max_gram_bytes
        self.solver = solver
        self.refit_solver = refit_solver

    # ---- argument checks (before any work) ----
    def _check(self):
        from sklearn.svm import SVC
        who = type(self).__name__
        if self.solver not in ("host", "device"):
            raise ValueError("%s: solver must be 'host' or 'device', got %r" % (who, self.solver))
        if self.refit_solver not in ("host", "device"):
            raise ValueError("%s: refit_solver must be 'host' or 'device', got %r" % (who, self.refit_solver))
        candidates, base = self._check_search(who, SVC, "SVC.score, GridSearchCV's default", _GRID_KEYS)
        for p in candidates:
            _check_kernel(who, p.get("kernel", base["kernel"]), p.get("gamma", base["gamma"]), p.get("C", base["C"]))
        return candidates, base

    def _check_data(self, X32, y):
        # what max_gram_bytes and n_jobs can raise in the stages of fit is raised here: before the search prints its header
        self._groups([], None, X32.shape[0]), self._threads(1)

    def _key(self, p, base):
        return _kernel_key(p.get("kernel", base["kernel"]), p.get("gamma", base["gamma"]))

    # the device entry points of the search and what turns the winner's fitted attributes into best_estimator_ (ProjMaskSearchSVC
    # has its own)
    _MAX_KEYS = 8                           # matrices per _gram / _smo call

    def _gram_of(self, s, keys):
        return _gram(s.X32, keys, self.device)

    def _smo_of(self, s, keys, plan):
        return _smo(s.X32, keys, plan, self.device)

    def _adopted(self, s, best, fitted, key):
        from sklearn.base import clone
        return _adopt(clone(self.estimator).set_params(**best), fitted, s.X32, key)

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
        plan = {"problems": np.array(problems, dtype=SMO_PROBLEM), "rows": _cat_i32(rows), "fits": np.array(fits, dtype=SMO_FIT),
                "test_rows": _cat_i32(test_rows), "test_y": _cat_i32(test_y), "n_classes": nc}
        return plan, on_device, host

    # ---- the stages of fit ----
    def _threads(self, n_fits):
        # joblib's convention (what GridSearchCV's n_jobs means): None -> 1, -1 -> every CPU this process may use, -2 -> all but one;
        # joblib counts the CPUs of the process's affinity mask and cgroup quota, not the whole machine's
        from joblib import effective_n_jobs
        return max(1, min(effective_n_jobs(self.n_jobs), n_fits))

    def _groups(self, candidates, base, N):
        """The distinct kernels of the grid in candidate order, in groups of at most 8 whose host copies stay under ``max_gram_bytes``."""
        mat_bytes = N * N * 8
        per = min(self._MAX_KEYS, int(self.max_gram_bytes // mat_bytes))
        if per < 1:
            raise ValueError(type(self).__name__ + ": one %d x %d kernel matrix takes %d bytes, more than max_gram_bytes=%d"
                             % (N, N, mat_bytes, self.max_gram_bytes))
        keys = []
        for p in candidates:
            k = self._key(p, base)
            if k not in keys:
                keys.append(k)
        return [keys[i:i + per] for i in range(0, len(keys), per)]

    def _fit_on_host(self, s, pool, mats, todo):
        """libsvm's fit and score of the (candidate, split) pairs ``todo`` on slices of the host matrices ``mats``, on the pool."""
        # The split fits run WITHOUT libsvm's Platt step (probability=False), whatever the base estimator says: the score is
        # accuracy of predict(), which does not use the Platt parameters, and the SMO solve is the same either way (libsvm fits
        # the pairwise models independently of the Platt cross-validation), so decision values and split scores are the bits
        # GridSearchCV gets -- at a sixth of the SMO work.  It also keeps libsvm's process-wide random generator (used only by
        # that cross-validation, outside the GIL) out of the concurrent fits.  The refit below keeps the base estimator's setting.
        def one(K, ci, si):
            tr, te = s.splits[si]
            est = self._svc(s.candidates[ci], s.base, "precomputed", probability=False)
            t0 = time.perf_counter()
            est.fit(K[np.ix_(tr, tr)], s.y[tr])
            t1 = time.perf_counter()
            acc = est.score(K[np.ix_(te, tr)], s.y[te])
            t2 = time.perf_counter()
            s.scores[ci, si], s.fit_t[ci, si], s.score_t[ci, si] = acc, t1 - t0, t2 - t1
            self._end_line(s.candidates[ci], si, len(s.splits), t2 - t0)

        jobs = [pool.submit(one, mats[self._key(s.candidates[ci], s.base)], ci, si) for ci, si in todo]
        for j in jobs:
            j.result()

    def _search_host(self, s, grp, pool):
        """One group of kernels searched on the host: its matrices by ``_gram``, every fit of its candidates on the pool."""
        todo = [(ci, si) for ci, p in enumerate(s.candidates) if self._key(p, s.base) in grp for si in range(len(s.splits))]
        mats = dict(zip(grp, self._gram_of(s, grp)))
        self._fit_on_host(s, pool, mats, todo)
        return _Matrices(mats, {}, {})

    def _search_device(self, s, grp, pool):
        """One group of kernels searched on the device: ``_smo_plan``'s batch by ``_smo``; what it leaves to the host is fitted there."""
        plan, on_device, todo = self._smo_plan(s.candidates, s.base, grp, s.splits, s.y)
        out = self._smo_of(s, grp, plan)
        fetch = {k: (lambda i=i, m=out["matrix"]: m(i)) for i, k in enumerate(grp)}
        resident = {k: (i, out["solve"]) for i, k in enumerate(grp)} if "solve" in out else {}
        for f, (ci, si) in enumerate(on_device):
            s.scores[ci, si] = float(out["correct"][f]) / len(s.splits[si][1])
            s.fit_t[ci, si] = out["solve_s"] / len(on_device)
            s.score_t[ci, si] = out["score_s"] / len(on_device)
            self._end_line(s.candidates[ci], si, len(s.splits), s.fit_t[ci, si] + s.score_t[ci, si])
        mats = {k: fetch[k]() for k in sorted({self._key(s.candidates[ci], s.base) for ci, _ in todo}, key=grp.index)}
        self._fit_on_host(s, pool, mats, todo)
        return _Matrices(mats, fetch, resident)

    def _refit(self, s, where):
        """The winner refitted on all rows, on its kernel matrix from ``where`` (the ``_Matrices`` of the last group) or computed again."""
        best = s.candidates[self.best_index_]
        key = self._key(best, s.base)
        if self.refit_solver == "device":
            # the winner's matrix where the search left it, or (host search, or a winner of an earlier group) computed again
            matrix, run = where.resident.get(key, (0, lambda plan: self._smo_of(s, [key], plan)))
            params = {k: s.base[k] for k in _FIT_CARRY}
            params["C"] = best.get("C", s.base["C"])
            t0 = time.perf_counter()
            fitted = _fit_batch(params, s.y, run, matrix)
            self.refit_time_ = time.perf_counter() - t0
        else:
            K = (where.host[key] if key in where.host else where.fetch[key]() if key in where.fetch
                 else self._gram_of(s, [key])[0])
            t0 = time.perf_counter()
            pre = self._svc(best, s.base, "precomputed").fit(K, s.y)
            self.refit_time_ = time.perf_counter() - t0
            params = pre.get_params()
            fitted = {k: v for k, v in vars(pre).items() if k not in params}
        self.best_estimator_ = self._adopted(s, best, fitted, key)

    def fit(self, X, y):
        candidates, base = self._check()
        X32, y, splits = self._setup(X, y, candidates)
        groups = self._groups(candidates, base, X32.shape[0])
        scores = np.zeros((len(candidates), len(splits)))         # with fit_t, score_t: (candidate, split) arrays the fits fill in
        s = SimpleNamespace(X32=X32, y=y, candidates=candidates, base=base, splits=splits, scores=scores, fit_t=np.zeros_like(scores),
                            score_t=np.zeros_like(scores))
        search = self._search_device if self.solver == "device" else self._search_host
        with ThreadPoolExecutor(max_workers=self._threads(len(candidates) * len(splits))) as pool:
            for grp in groups:
                where = search(s, grp, pool)            # the refit reads that of the last group
        self._finish(candidates, len(splits), s.fit_t, s.score_t, s.scores)
        if self.refit:
            self._refit(s, where)
        self.classes_ = np.unique(y)
        return self


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
    return _log_best(grid_search)


# ---- ProjMaskSearchSVC: the projection mask searched with the grid, and the reference's search with it -----------------------------
def _all_proj_masks():
    from .common import ProjMask
    return [ProjMask(bool(b & 1), bool(b & 2), bool(b & 4)) for b in range(1, 8)]


class ProjMaskSearchSVC(GridSearchSVC):
    """``GridSearchSVC`` over projection masks x ``param_grid``: the reference's "which projections" hyperparameter searched in one
    fit instead of one ``GridSearchSVC`` per mask on a column subset.

    ``fit(X, y)`` takes the FULL rows, the concatenation of ``segments`` = (xz, yz, xy) feature counts.  They are uploaded once, one
    ``rml_gram_segments`` pass forms the inner products and squared norms of every projection, and every mask x kernel matrix is
    composed from those (``rml_gram_compose``: the products of a mask are the sums of its projections') in groups that stay under
    ``max_gram_bytes``; each group is searched as ``GridSearchSVC`` searches a group of kernels (``solver`` / ``refit_solver`` as
    there).  Candidates are ``proj_masks`` (outer, in the given order; default: the seven non-empty masks by ``common._mask_bits``)
    x ``ParameterGrid(param_grid)`` (inner); ``cv_results_`` has ``param_proj_mask`` and ``"proj_mask"`` in every ``params`` dict,
    ranks run over all candidates and the first best wins.  ``best_proj_mask_`` is the winner's mask, ``best_params_`` its grid
    point without the mask, and ``best_estimator_`` a genuine ``SVC`` fitted on the winning mask's columns.  ``predict``,
    ``decision_function``, ``predict_proba`` and ``score`` take full rows and select those columns."""

    _MAX_KEYS = 1 << 30                     # rml_gram_compose has no cap: max_gram_bytes alone sizes a group

    def __init__(self, estimator, param_grid, segments, proj_masks=None, cv=5, n_jobs=4, refit=True, device=None,
                 max_gram_bytes=8 << 30, scoring=None, verbose=0, solver="host", refit_solver="host"):
        super().__init__(estimator, param_grid, cv, n_jobs, refit, device, max_gram_bytes, scoring, verbose, solver, refit_solver)
        self.segments = segments
        self.proj_masks = proj_masks

    def _segments(self):
        seg = tuple(int(v) for v in self.segments)
        if len(seg) != 3 or any(v < 0 for v in seg):
            raise ValueError("ProjMaskSearchSVC: segments are the three feature counts (xz, yz, xy), got %r" % (self.segments,))
        return seg

    def _masks(self):
        from .common import ProjMask, _mask_bits
        seg = self._segments()
        masks = _all_proj_masks() if self.proj_masks is None else [ProjMask(*(bool(v) for v in m)) for m in self.proj_masks]
        for m in masks:
            _mask_bits(m)                   # raises on a mask that selects no projection
            if any(m[i] and seg[i] == 0 for i in range(3)):
                raise ValueError("ProjMaskSearchSVC: %r selects a projection of zero length (segments %r)" % (m, seg))
        return masks

    def _cols(self, mask):
        start = np.concatenate([[0], np.cumsum(self._segments())])
        return np.concatenate([np.arange(start[i], start[i + 1]) for i in range(3) if mask[i]])

    def _check(self):
        grid, base = super()._check()
        return [dict(p, proj_mask=m) for m in self._masks() for p in grid], base

    def _check_data(self, X32, y):
        if X32.shape[1] != sum(self._segments()):
            raise ValueError("ProjMaskSearchSVC: X has %d features, segments %r add up to %d" % (X32.shape[1], self._segments(),
                                                                                               sum(self._segments())))
        super()._check_data(X32, y)

    def _key(self, p, base):
        from .common import _mask_bits
        return (_mask_bits(p["proj_mask"]),) + super()._key(p, base)

    def _gram_of(self, s, keys):
        return _gram_masks(s.X32, self._segments(), keys, self.device)

    def _smo_of(self, s, keys, plan):
        return _smo_masks(s.X32, self._segments(), keys, plan, self.device)

    def _adopted(self, s, best, fitted, key):
        from sklearn.base import clone
        params = {k: v for k, v in best.items() if k != "proj_mask"}
        rows = np.ascontiguousarray(s.X32[:, self._cols(best["proj_mask"])])
        return _adopt(clone(self.estimator).set_params(**params), fitted, rows, key[1:])

    def _finish(self, candidates, n_splits, fit_t, score_t, scores):
        super()._finish(candidates, n_splits, fit_t, score_t, scores)
        best = candidates[self.best_index_]
        self.best_proj_mask_ = best["proj_mask"]
        self.best_params_ = {k: v for k, v in best.items() if k != "proj_mask"}

    def fit(self, X, y):
        try:
            return super().fit(X, y)
        finally:
            _release_segments()             # the segment products were resident for the whole fit, and no longer

    def _best_rows(self, X):
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != sum(self._segments()):
            raise ValueError("ProjMaskSearchSVC: expected full rows of %d features, got an array of shape %r"
                             % (sum(self._segments()), X.shape))
        return X[:, self._cols(self.best_proj_mask_)]

    def predict(self, X):
        return self.best_estimator_.predict(self._best_rows(X))

    def decision_function(self, X):
        return self.best_estimator_.decision_function(self._best_rows(X))

    def predict_proba(self, X):
        return self.best_estimator_.predict_proba(self._best_rows(X))

    def score(self, X, y):
        return self.best_estimator_.score(self._best_rows(X), y)


def find_best_proj_mask_svm_estimator(X, y, cv, random_seed, segments, proj_masks=None, solver="host", refit_solver="host"):
    """``find_best_svm_estimator`` with the projection mask searched as well (the reference's README: "choosing the optimal
    combination as a training hyperparameter"): the same grid, base estimator and log lines over ``proj_masks`` (default: all
    seven) of the full rows ``X`` = concat of ``segments`` (xz, yz, xy) columns (ProjMaskSearchSVC).

    Returns:
        (optimized svm estimator, fitted on the winning mask's columns; that ProjMask).
    """
    from sklearn import svm
    print('\n Finding best svm estimator and projection mask...')
    Cs = [0.01, 0.1, 1, 10, 100]
    gammas = [0.001, 0.01, 0.1, 1, 10]
    param_grid = [
        {'C': Cs, 'kernel': ['linear']},
        {'C': Cs, 'gamma': gammas, 'kernel': ['rbf']}
    ]
    init_est = svm.SVC(probability=True, class_weight='balanced',
                       random_state=random_seed, cache_size=1000, verbose=False)
    grid_search = ProjMaskSearchSVC(estimator=init_est, param_grid=param_grid, segments=segments, proj_masks=proj_masks, verbose=2,
                                    n_jobs=4, cv=cv, solver=solver, refit_solver=refit_solver)
    grid_search.fit(X, y)
    estimator = _log_best(grid_search)
    logger.info('\n Best projection mask:')
    logger.info(grid_search.best_proj_mask_)
    return estimator, grid_search.best_proj_mask_


# ---- GridSearchSGD and the reference's find_best_sgd_svm_estimator -----------------------------------------------------------------
_SGD_GRID_KEYS = ("alpha", "penalty", "l1_ratio", "average", "max_iter", "tol", "n_iter_no_change", "shuffle")


class GridSearchSGD(_GridSearch):
    """``GridSearchCV(SGDClassifier(loss='log_loss'), param_grid)`` on the GPU: the counterpart of ``GridSearchSVC`` for the
    reference's default model, with the same subset of ``GridSearchCV``'s surface (``fit(X, y)``, ``best_estimator_``,
    ``best_params_``, ``best_score_``, ``best_index_``, ``cv_results_``, ``n_splits_``, ``refit_time_``, ``scorer_``: accuracy).

    The rows are uploaded once.  Every candidate (``ParameterGrid`` order) x split x class is one problem of ONE ``rml_sgd_solve``
    call, every held-out row is scored by ONE ``rml_sgd_score`` call from the weights where the solve left them, and the winner is
    refitted on all rows by one more solve on the resident rows (``fit_sgd``'s path).  The grid may vary ``alpha``, ``penalty``,
    ``l1_ratio``, ``average``, ``max_iter``, ``tol``, ``n_iter_no_change`` and ``shuffle``; everything else is the base estimator's,
    under ``fit_sgd``'s restrictions.  ``class_weight`` is formed per fold as scikit-learn forms it.  The batch has no per-fit
    times: ``fit_time`` / ``score_time`` are the batch's solve / score time divided evenly among its fits."""

    def __init__(self, estimator, param_grid, cv=5, refit=True, device=None, scoring=None, verbose=0, n_jobs=None):
        # n_jobs is accepted for GridSearchCV's signature; the batch is one launch whatever it says
        super().__init__(estimator, param_grid, cv, n_jobs, refit, device, scoring, verbose)

    def _check(self):
        from sklearn.linear_model import SGDClassifier
        candidates, base = self._check_search("GridSearchSGD", SGDClassifier, "GridSearchCV's default for a classifier", _SGD_GRID_KEYS)
        prms = [_sgd_params(dict(base, **p), "GridSearchSGD") for p in candidates]
        return candidates, base, prms

    def _check_data(self, X32, y):
        if not 2 <= len(np.unique(y)) <= 8:
            raise ValueError("GridSearchSGD takes 2..8 classes, got %d" % len(np.unique(y)))

    def _plan(self, prms, base, splits, y):
        """The batch of the search for ``_sgd``: per candidate and split one fit of one problem per class (one for two classes), on
        the split's shared row list and per-class label lists.  Returns (plan, [(ci, si) of fit f])."""
        from sklearn.utils.class_weight import compute_class_weight
        classes = np.unique(y)
        nc = len(classes)
        yi = np.searchsorted(classes, y).astype(np.int32)
        positives = [1] if nc == 2 else list(range(nc))
        rows, ys, test_rows, test_y, per_split = [], [], [], [], []
        n_rows = n_y = 0
        for tr, te in splits:
            if len(np.unique(yi[tr])) < nc:
                raise NotImplementedError("GridSearchSGD: a split whose training rows miss a class (scikit-learn fits a model of fewer "
                                          "classes there)")
            _sgd_check_rows("GridSearchSGD", len(tr))
            w = compute_class_weight(base["class_weight"], classes=classes, y=y[tr])
            y_offs = []
            for c in positives:
                ys.append((yi[tr] == c).astype(np.int32))
                y_offs.append(n_y)
                n_y += len(tr)
            per_split.append((n_rows, y_offs, w))
            rows.append(tr)
            n_rows += len(tr)
        problems, fits, which = [], [], []
        n_test = 0
        for ci, prm in enumerate(prms):
            for si, (tr, te) in enumerate(splits):
                rows_off, y_offs, w = per_split[si]
                seeds = _sgd_seeds(base["random_state"], nc)
                fits.append((len(problems), len(te), n_test))
                which.append((ci, si))
                test_rows.append(te)
                test_y.append(yi[te])
                n_test += len(te)
                for k, c in enumerate(positives):
                    problems.append(_sgd_problem(prm, len(tr), seeds[k], rows_off, y_offs[k], len(problems), w[c],
                                                 w[0] if nc == 2 else 1.0))
        plan = {"problems": np.array(problems, dtype=SGD_PROBLEM), "rows": _cat_i32(rows), "y": _cat_i32(ys), "n_out": len(problems),
                "fits": np.array(fits, dtype=SGD_FIT), "test_rows": _cat_i32(test_rows), "test_y": _cat_i32(test_y), "n_classes": nc}
        return plan, which

    def fit(self, X, y):
        import warnings
        from sklearn.base import clone
        from sklearn.exceptions import ConvergenceWarning
        candidates, base, prms = self._check()
        X32, y, splits = self._setup(X, y, candidates)
        n_splits = len(splits)
        plan, which = self._plan(prms, base, splits, y)
        out = _sgd(X32, plan, self.device)
        _sgd_check_overflow(out)
        probs = plan["problems"]
        if ((probs["tol"] > -np.inf) & (out["n_iter"][probs["out"]] == probs["max_iter"])).any():
            warnings.warn(_SGD_MAX_ITER, ConvergenceWarning)
        scores = np.zeros((len(candidates), n_splits))
        fit_t = np.full_like(scores, out["solve_s"] / len(which))
        score_t = np.full_like(scores, out["score_s"] / len(which))
        for f, (ci, si) in enumerate(which):
            scores[ci, si] = float(out["correct"][f]) / len(splits[si][1])
            self._end_line(candidates[ci], si, n_splits, fit_t[ci, si] + score_t[ci, si])
        self._finish(candidates, n_splits, fit_t, score_t, scores)
        self.solve_time_, self.score_time_ = out["solve_s"], out["score_s"]
        if self.refit:
            est = clone(self.estimator).set_params(**self.best_params_)
            _sgd_prepare(est, "GridSearchSGD")
            t0 = time.perf_counter()
            self.best_estimator_ = _sgd_fit(est, X32, y, out["solve"], "GridSearchSGD")
            self.refit_time_ = time.perf_counter() - t0
        self.classes_ = np.unique(y)
        return self


def find_best_sgd_svm_estimator(X, y, cv, random_seed, device=None):
    """Exhaustive search over specified parameter values for svm using sgd (train.py:350-381, the same grid, base estimator and
    log lines), every fit of the search and the refit on the GPU (GridSearchSGD).

    Returns:
        optimized svm estimator.
    """
    from sklearn import linear_model
    max_iter = max(np.ceil(10**6 / len(X)), 1000)
    small_alphas = [10.0e-08, 10.0e-09, 10.0e-10]
    alphas = [10.0e-04, 10.0e-05, 10.0e-06, 10.0e-07]
    l1_ratios = [0.075, 0.15, 0.30]
    param_grid = [
        {'alpha': alphas, 'penalty': ['l1', 'l2'], 'average': [False]},
        {'alpha': alphas, 'penalty': ['elasticnet'], 'average': [False],
         'l1_ratio': l1_ratios},
        {'alpha': small_alphas, 'penalty': ['l1', 'l2'], 'average': [True]},
        {'alpha': small_alphas, 'penalty': ['elasticnet'], 'average': [True],
         'l1_ratio': l1_ratios}
    ]
    init_est = linear_model.SGDClassifier(loss='log', max_iter=max_iter,
                                          random_state=random_seed, n_jobs=-1, warm_start=True)
    grid_search = GridSearchSGD(estimator=init_est, param_grid=param_grid, verbose=2, n_jobs=-1, cv=cv, device=device)
    grid_search.fit(X, y)
    return _log_best(grid_search)


# ---- the flows of the reference: sgd_fit and svc_fit, with their class balancing and feature rows ----------------------------------
def balance_indices(labels):
    """The index form of ``balance_classes``: the positions it takes its balanced set from, in its order, or None where the
    labels are balanced already (it then returns its input)."""
    import collections
    from sklearn import utils
    labels = np.asarray(labels)
    mc = collections.Counter(labels.tolist()).most_common()
    if len(set(c for _, c in mc)) == 1:
        return None
    majority = mc[0][1]
    # utils.resample(a, ...) is a[random_state.randint(0, len(a), n_samples)]: drawing on the index array takes the same rows
    return np.concatenate([utils.resample(np.nonzero(labels == c)[0], replace=True, n_samples=majority, random_state=RANDOM_SEED)
                           for c, _ in mc])


def balance_classes(labels, data):
    """Balance classes (train.py:230-274): every class upsampled with replacement to the size of the most frequent one, the classes
    in ``Counter.most_common`` order, the draws those of ``utils.resample(..., random_state=RANDOM_SEED)`` on the host.  ``data``:
    host rows (NumPy indexing) or a CUDA tensor (one gather).  Already-balanced input is returned as it is."""
    idx = balance_indices(labels)
    if idx is None:
        return labels, data
    labels = np.asarray(labels)
    try:
        import torch
        if isinstance(data, torch.Tensor):
            return labels[idx], data[torch.as_tensor(idx, dtype=torch.long, device=data.device)]
    except ImportError:   # pragma: no cover - torch is part of the image
        pass
    return labels[idx], np.asarray(data)[idx]


def _feature_rows(samples, proj_mask, device=None):
    """``common.process_samples`` at zoom 1 for a list of projection tuples whose planes are host arrays or CUDA tensors (the output
    of ``DataGenerator.augment_dataset``), to DEVICE rows: the host planes go up in one copy per projection, the device planes are
    taken where they are, and ``rml_assemble_features`` writes the rows."""
    import torch
    from . import common
    lib = _lib.load()
    dev = _lib.device_of(device)
    samples = list(samples)
    n = len(samples)
    if n == 0:
        raise ValueError("no samples")
    with torch.cuda.device(dev):
        planes = []
        for i in range(3):
            if not proj_mask[i]:
                planes.append(None)
                continue
            shp = tuple(int(v) for v in samples[0][i].shape)
            if len(shp) != 2 or any(tuple(int(v) for v in s[i].shape) != shp for s in samples):
                raise ValueError("setting an array element with a sequence: ragged projection shapes")
            out = torch.empty((n,) + shp, dtype=torch.float32, device=dev)
            host = [j for j, s in enumerate(samples) if not isinstance(s[i], torch.Tensor)]
            there = [j for j, s in enumerate(samples) if isinstance(s[i], torch.Tensor)]
            if host:
                out[torch.as_tensor(host, device=dev)] = torch.from_numpy(np.stack([np.asarray(samples[j][i], dtype=np.float32)
                                                                                   for j in host])).to(dev)
            if there:
                out[torch.as_tensor(there, device=dev)] = torch.stack([samples[j][i].to(device=dev, dtype=torch.float32) for j in there])
            planes.append(out)
        X = planes[0].shape[1] if planes[0] is not None else (planes[2].shape[1] if planes[2] is not None else 1)
        Z = planes[0].shape[2] if planes[0] is not None else (planes[1].shape[2] if planes[1] is not None else 1)
        Y = planes[1].shape[1] if planes[1] is not None else (planes[2].shape[2] if planes[2] is not None else 1)
        for i, want in enumerate([(X, Z), (Y, Z), (X, Y)]):
            if planes[i] is not None and tuple(planes[i].shape[1:]) != want:
                raise ValueError("projection shapes are inconsistent: got %s for plane %d, expected %s" % (tuple(planes[i].shape[1:]), i, want))
        bits = common._mask_bits(proj_mask)
        D = int(lib.rml_feature_len(X, Y, Z, bits))
        feat = torch.empty((n, D), dtype=torch.float32, device=dev)
        _lib.check(lib.rml_assemble_features(_lib.context(dev), _lib.ptr(planes[0]), _lib.ptr(planes[1]), _lib.ptr(planes[2]), n, X, Y, Z,
                                             0.0, bits, _lib.ptr(feat), D, _lib.stream_ptr(dev)), "rml_assemble_features")
    return feat


def _online_learn_steps(n):
    """train.py:414: the partial_fit calls of --online_learn over a training set of n rows."""
    return int(max(np.ceil(10**6 / n), 1000))


def _augment_steps(sample_of, labels, n_samples, batch_size):
    """The partial_fit calls of one augment epoch (train.py:427-438): per slice of ``batch_size`` samples the augmented rows whose
    sample lies in it, balanced as ``balance_classes`` balances the batch.  ``len(xc) / batch_size`` batches, as train.py:437 counts."""
    steps = []
    for b in range(int(np.ceil(n_samples / batch_size))):
        jobs = np.nonzero(np.asarray(sample_of) // batch_size == b)[0]
        if len(jobs) == 0:
            continue
        idx = balance_indices(labels[jobs])
        steps.append(jobs if idx is None else jobs[idx])
    return steps


def sgd_fit(train, test, proj_mask, online_learn, svm_model, epochs, folds=5, batch_size=32, device=None):
    """Fit SVM using SGD on data set (train.py:324-440, the same arguments) with every fit on the GPU.

    The features are made once and balanced; then either the grid search (``find_best_sgd_svm_estimator``) or, for
    ``online_learn``, the pickled classifier ``svm_model`` (a path or an open file) and its ``max(ceil(1e6 / n), 1000)`` identical
    partial fits in ONE ``partial_fit_sgd_steps`` call.  Then per augment epoch: one ``DataGenerator.augment_dataset`` call (the
    draws in the reference's order, batch by batch), one feature pass to device rows, per batch the balanced row list of the
    augmented samples that come from it, and one ``partial_fit_sgd_steps`` call that predicts ``X_test`` after every step -- one wait
    per epoch; the per-batch accuracies are logged at debug level afterwards.

    Returns:
        estimator: Estimator that was chosen by grid search.
    """
    import pickle
    from sklearn import model_selection
    from .augment import DataGenerator
    from .svm import from_sklearn
    X_train, y_train = train
    X_test, y_test = test
    y_train, y_test = np.asarray(y_train), np.asarray(y_test)
    if epochs:
        xc = list(X_train)
        yc = y_train.copy()
    logger.info('Generating feature vectors.')
    Xd_test = _feature_rows(X_test, proj_mask, device)
    Xd = _feature_rows(X_train, proj_mask, device)
    logger.info(f'Feature vector length: {Xd.shape[1]}')
    logger.info('Balancing classes.')
    y_bal, Xd = balance_classes(y_train, Xd)
    if not online_learn:
        logger.info('Running best fit with new data.')
        skf = model_selection.StratifiedKFold(n_splits=folds)
        Xh = Xd.cpu().numpy()
        clf = find_best_sgd_svm_estimator(Xh, y_bal, list(skf.split(Xh, y_bal)), RANDOM_SEED, device=device)
    else:
        logger.info('Running partial fit with new data.')
        if hasattr(svm_model, "read"):
            clf = pickle.load(svm_model)
        else:
            with open(svm_model, 'rb') as fp:
                clf = pickle.load(fp)
        everything = np.arange(len(y_bal))
        clf, _ = partial_fit_sgd_steps(clf, Xd, y_bal, [everything] * _online_learn_steps(len(y_bal)), device=device)
    if epochs:
        logger.info(f'Running partial fit with augmented data (epochs: {epochs}).')
        if logger.isEnabledFor(logging.DEBUG):
            y_predicted = from_sklearn(clf).predict(Xd_test)
            logger.debug(f'Un-augmented accuracy: {float(np.mean(y_predicted == y_test))}.')
        data_gen = DataGenerator(rotation_range=5.0, zoom_range=0.2, noise_sd=0.1, balance=True, device=device)
        classes = np.unique(y_bal)
        for e in range(epochs):
            logger.debug(f'Augment epoch: {e}.')
            tuples, labels, sample_of = data_gen.augment_dataset(xc, yc, return_samples=True)
            Xe = _feature_rows(list(tuples) + list(X_test), proj_mask, device)
            steps = _augment_steps(sample_of, labels, len(xc), batch_size)
            held_out = (np.arange(len(labels), len(labels) + len(y_test)), y_test)
            clf, acc = partial_fit_sgd_steps(clf, Xe, np.concatenate((labels, y_test)), steps, classes=classes, test=held_out,
                                             device=device)
            for batch, a in enumerate(acc):
                logger.debug(f'Augment batch: {batch}.')
                logger.debug(f'Augmented accuracy: {a}.')
    return clf


def _svc_training_set(train, epochs, device):
    """The projection tuples and labels ``svc_fit`` searches on (train.py:442-520): the training set augmented ``epochs`` times on the
    GPU, with the reference's 1e-6 scale check.  Nothing here depends on the projection mask."""
    import torch
    from .augment import DataGenerator
    X_train, y_train = train
    X_train = list(X_train)
    y_train = np.asarray(y_train)
    if epochs:
        data_gen = DataGenerator(rotation_range=15.0, zoom_range=0.3, noise_sd=0.2, device=device)
        logger.info('Augmenting data set.')
        logger.info(f'Original number of training samples: {y_train.shape[0]}')
        xc, yc = list(X_train), y_train.copy()
        y_parts = [y_train]
        for e in range(epochs):
            logger.debug(f'epoch: {e}')
            tuples, labels = data_gen.augment_dataset(xc, yc)
            X_train.extend(tuples)
            y_parts.append(labels)
        # Sanity check if augmentation introduced a scaling problem.
        top = max(float(p.max()) if isinstance(p, torch.Tensor) else float(np.max(p)) for t in X_train for p in t)
        assert abs(top - 1.0) < 1e-6, 'scale error'
        y_train = np.concatenate(y_parts).astype(np.int8)
        logger.info(f'Augmented number of training samples: {y_train.shape[0]}')
    return X_train, y_train


def svc_fit(train, proj_mask, epochs, folds=5, batch_size=32, solver="host", refit_solver="host", device=None):
    """Fit SVM using SVC on data set (train.py:442-545): the training set augmented ``epochs`` times on the GPU (one
    ``DataGenerator.augment_dataset`` call per epoch; ``batch_size`` only sliced the reference's loop, the draws are the same
    stream), the 1e-6 scale check, the features to device rows, ``balance_classes`` and ``find_best_svm_estimator``
    (``solver`` / ``refit_solver`` as there).

    Returns:
        estimator: Estimator that was chosen by grid search.
    """
    from sklearn import model_selection
    X_train, y_train = _svc_training_set(train, epochs, device)
    logger.info('Generating feature vectors from radar projections.')
    Xd = _feature_rows(X_train, proj_mask, device)
    logger.info(f'Feature vector length: {Xd.shape[1]}')
    logger.info('Balancing classes.')
    y_train, Xd = balance_classes(y_train, Xd)
    skf = model_selection.StratifiedKFold(n_splits=folds)
    logger.info('Finding best classifier.')
    Xh = Xd.cpu().numpy()
    return find_best_svm_estimator(Xh, y_train, list(skf.split(Xh, y_train)), RANDOM_SEED, solver=solver, refit_solver=refit_solver)


def svc_fit_masks(train, epochs, proj_masks=None, folds=5, batch_size=32, solver="host", refit_solver="host", device=None):
    """``svc_fit`` with the projection mask chosen by the search: the same augmentation, scale check, ``balance_classes`` and
    ``StratifiedKFold`` (none depends on the mask) on rows assembled ONCE from all three projections, then
    ``find_best_proj_mask_svm_estimator`` over ``proj_masks`` (default: all seven) with the segments taken from the samples' plane
    shapes.

    Returns:
        (estimator chosen by the search, fitted on its mask's columns; that ProjMask).
    """
    from sklearn import model_selection
    from .common import ProjMask
    X_train, y_train = _svc_training_set(train, epochs, device)
    segments = tuple(int(np.prod(tuple(X_train[0][i].shape))) for i in range(3))
    logger.info('Generating feature vectors from radar projections.')
    Xd = _feature_rows(X_train, ProjMask(True, True, True), device)
    logger.info(f'Feature vector length: {Xd.shape[1]}')
    logger.info('Balancing classes.')
    y_train, Xd = balance_classes(y_train, Xd)
    skf = model_selection.StratifiedKFold(n_splits=folds)
    logger.info('Finding best classifier and projection mask.')
    Xh = Xd.cpu().numpy()
    return find_best_proj_mask_svm_estimator(Xh, y_train, list(skf.split(Xh, y_train)), RANDOM_SEED, segments, proj_masks=proj_masks,
                                             solver=solver, refit_solver=refit_solver)


# ---- calibration and evaluation ----------------------------------------------------------------------------------------------------
def calibrate_prefit(clf, X_val, y_val):
    """``CalibratedClassifierCV(clf, cv='prefit').fit(X_val, y_val)`` (train.py:722-724) for a fitted SVC or SGDClassifier: the
    decision values of the validation rows come from the GPU twin (``from_sklearn(clf).decision_function``), the two-parameter
    sigmoid fits from scikit-learn's own ``_fit_calibrator`` on the host (some hundred values per class), and the result is a
    genuine ``CalibratedClassifierCV`` that pickles and that ``from_sklearn`` takes."""
    from sklearn.calibration import CalibratedClassifierCV, _fit_calibrator
    from .svm import from_sklearn
    y_val = np.asarray(y_val)
    predictions = np.asarray(from_sklearn(clf).decision_function(X_val), dtype=np.float64)
    if predictions.ndim == 1:
        predictions = predictions.reshape(-1, 1)
    if len(predictions) != len(y_val):
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (len(predictions), len(y_val)))
    cal = CalibratedClassifierCV(estimator=clf, cv="prefit")
    cal.classes_ = clf.classes_
    cal.calibrated_classifiers_ = [_fit_calibrator(clf, predictions, y_val, cal.classes_, cal.method, None)]
    if hasattr(clf, "n_features_in_"):
        cal.n_features_in_ = clf.n_features_in_
    return cal


def evaluate_model(model, X_test, y_test, target_names, cm_name=None):
    """Generate model confusion matrix and classification report (train.py:215-228): the labels come from the GPU model
    (``from_sklearn(model)`` unless it is one already), accuracy, confusion matrix and report from ``sklearn.metrics``; the
    figure of train.py:293-322 is drawn and saved only when ``cm_name`` is given.  Returns (accuracy, confusion matrix, report)."""
    from sklearn import metrics
    from .svm import from_sklearn, _Base
    gpu = model if isinstance(model, _Base) else from_sklearn(model)
    y_pred = gpu.predict(X_test)
    acc = metrics.accuracy_score(y_test, y_pred)
    logger.info(f'Accuracy: {acc}')
    cm = metrics.confusion_matrix(y_test, y_pred)
    logger.info(f'Confusion matrix:\n{cm}')
    if cm_name is not None:
        import itertools
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        figure = plt.figure(figsize=(8, 8))
        ax = plt.gca()
        im = ax.imshow(cm, interpolation='nearest', cmap=plt.cm.Blues)
        plt.title('Confusion matrix')
        plt.colorbar(im, fraction=0.046, pad=0.04)
        tick_marks = np.arange(len(target_names))
        plt.xticks(tick_marks, target_names, rotation=45)
        plt.yticks(tick_marks, target_names)
        norm = np.around(cm.astype('float') / cm.sum(axis=1)[:, np.newaxis], decimals=2)
        threshold = norm.max() / 2.
        for i, j in itertools.product(range(norm.shape[0]), range(norm.shape[1])):
            plt.text(j, i, norm[i, j], horizontalalignment='center', color='white' if norm[i, j] > threshold else 'black')
        plt.tight_layout()
        plt.ylabel('True label')
        plt.xlabel('Predicted label')
        logger.info(f'Saving confusion matrix plot to: {cm_name}')
        figure.savefig(cm_name)
        figure.clf()
        plt.close(figure)
    cls_report = metrics.classification_report(y_test, y_pred, target_names=target_names)
    logger.info(f'Classification report:\n{cls_report}')
    return acc, cm, cls_report
