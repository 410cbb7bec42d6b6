"""Shared helpers of the device SMO tests (tests/test_smo_cpu.py, tests/test_smo_gpu.py): a NumPy float64 twin of libsvm's
``Solver::Solve`` as scikit-learn ships it (test oracle only, like ``grid_search_common.numpy_gram``: the package ships no host
solver), the problems the tests run, and scikit-learn's own fits of them, made once per session."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
sys.path.pop(0)

INF = np.inf
TAU = 1e-12


def solve(K, y, Cv, eps=1e-3, shrinking=True, max_iter=-1):
    """sklearn/svm/src/libsvm/svm.cpp Solver::Solve for C-SVC (p = -1) on the precomputed matrix K, the per-element loops as array
    operations.  y: +1 / -1, Cv: per-row C.  Returns (alpha, rho, n_iter, shrink passes, stopped early)."""
    l = len(y)
    y = np.asarray(y).astype(np.int64).copy()
    C = np.asarray(Cv, dtype=np.float64).copy()
    p = -np.ones(l)
    alpha = np.zeros(l)
    aset = np.arange(l)
    G_ = p.copy()
    Gb = np.zeros(l)
    st = np.zeros(l, np.int8)                       # 0 lower bound, 1 upper bound, 2 free
    act = l
    unshrink = False

    def upd(i):
        st[i] = 1 if alpha[i] >= C[i] else (0 if alpha[i] <= 0 else 2)

    def Qrow(i, n):                                 # SVC_Q::get_Q: rounded to Qfloat
        return np.float32((y[i] * y[:n]) * K[aset[i], aset[:n]]).astype(np.float64)

    def QD(n):
        return K[aset[:n], aset[:n]]

    def swap(i, j):
        for a in (y, G_, st, alpha, p, aset, Gb, C):
            a[i], a[j] = a[j], a[i]

    def recon():
        if act == l:
            return
        G_[act:] = Gb[act:] + p[act:]
        for i in range(act):
            if st[i] == 2:
                G_[act:] += alpha[i] * Qrow(i, l)[act:]

    def select():
        n = act
        yy, g, s = y[:n], G_[:n], st[:n]
        up = ((yy == 1) & (s != 1)) | ((yy == -1) & (s != 0))
        v = np.where(yy == 1, -g, g)
        if not up.any():
            return 1, -1, -1
        Gmax = v[up].max()
        i = np.nonzero(up & (v == Gmax))[0][-1]     # >= while scanning upwards: the last of equal values
        Qi = Qrow(i, n)
        low = ((yy == 1) & (s != 0)) | ((yy == -1) & (s != 1))
        gv = np.where(yy == 1, g, -g)
        Gmax2 = gv[low].max() if low.any() else -INF
        gd = Gmax + gv
        cand = low & (gd > 0)
        if Gmax + Gmax2 < eps or not cand.any():
            return 1, -1, -1
        qd = QD(n)
        quad = np.where(yy == 1, qd[i] + qd - 2.0 * y[i] * Qi, qd[i] + qd + 2.0 * y[i] * Qi)
        obj = np.where(quad > 0, -(gd * gd) / np.where(quad > 0, quad, 1.0), -(gd * gd) / TAU)
        obj = np.where(cand, obj, INF)
        j = np.nonzero(cand & (obj == obj.min()))[0][-1]
        return 0, i, j

    def be_shrunk(i, g1, g2):
        if st[i] == 1:
            return (-G_[i] > g1) if y[i] == 1 else (-G_[i] > g2)
        if st[i] == 0:
            return (G_[i] > g2) if y[i] == 1 else (G_[i] > g1)
        return False

    def shrink():
        nonlocal act, unshrink
        n = act
        yy, g, s = y[:n], G_[:n], st[:n]
        a1 = np.concatenate([-g[(yy == 1) & (s != 1)], g[(yy == -1) & (s != 0)], [-INF]]).max()
        a2 = np.concatenate([g[(yy == 1) & (s != 0)], -g[(yy == -1) & (s != 1)], [-INF]]).max()
        if not unshrink and a1 + a2 <= eps * 10:
            unshrink = True
            recon()
            act = l
        i = 0
        while i < act:
            if be_shrunk(i, a1, a2):
                act -= 1
                while act > i:
                    if not be_shrunk(act, a1, a2):
                        swap(i, act)
                        break
                    act -= 1
            i += 1

    it = 0
    counter = min(l, 1000) + 1
    nshr = 0
    stopped = False
    while True:
        if max_iter != -1 and it >= max_iter:
            stopped = True
            break
        counter -= 1
        if counter == 0:
            counter = min(l, 1000)
            if shrinking:
                shrink()
                nshr += 1
        r, i, j = select()
        if r:
            recon()
            act = l
            r, i, j = select()
            if r:
                break
            counter = 1
        it += 1
        Qi, Qj = Qrow(i, act), Qrow(j, act)
        Ci, Cj = C[i], C[j]
        oi, oj = alpha[i], alpha[j]
        qd = QD(act)
        if y[i] != y[j]:
            q = qd[i] + qd[j] + 2 * Qi[j]
            if q <= 0:
                q = TAU
            d = (-G_[i] - G_[j]) / q
            diff = alpha[i] - alpha[j]
            alpha[i] += d
            alpha[j] += d
            if diff > 0:
                if alpha[j] < 0:
                    alpha[j] = 0
                    alpha[i] = diff
            else:
                if alpha[i] < 0:
                    alpha[i] = 0
                    alpha[j] = -diff
            if diff > Ci - Cj:
                if alpha[i] > Ci:
                    alpha[i] = Ci
                    alpha[j] = Ci - diff
            else:
                if alpha[j] > Cj:
                    alpha[j] = Cj
                    alpha[i] = Cj + diff
        else:
            q = qd[i] + qd[j] - 2 * Qi[j]
            if q <= 0:
                q = TAU
            d = (G_[i] - G_[j]) / q
            sm = alpha[i] + alpha[j]
            alpha[i] -= d
            alpha[j] += d
            if sm > Ci:
                if alpha[i] > Ci:
                    alpha[i] = Ci
                    alpha[j] = sm - Ci
            else:
                if alpha[j] < 0:
                    alpha[j] = 0
                    alpha[i] = sm
            if sm > Cj:
                if alpha[j] > Cj:
                    alpha[j] = Cj
                    alpha[i] = sm - Cj
            else:
                if alpha[i] < 0:
                    alpha[i] = 0
                    alpha[j] = sm
        dai, daj = alpha[i] - oi, alpha[j] - oj
        G_[:act] += Qi * dai + Qj * daj
        ui, uj = st[i] == 1, st[j] == 1
        upd(i)
        upd(j)
        if ui != (st[i] == 1):
            if ui:
                Gb -= Ci * Qrow(i, l)
            else:
                Gb += Ci * Qrow(i, l)
        if uj != (st[j] == 1):
            if uj:
                Gb -= Cj * Qrow(j, l)
            else:
                Gb += Cj * Qrow(j, l)
    nfree, ub, lb, sf = 0, INF, -INF, 0.0
    for k in range(act):
        yG = y[k] * G_[k]
        if st[k] == 1:
            if y[k] == -1:
                ub = min(ub, yG)
            else:
                lb = max(lb, yG)
        elif st[k] == 0:
            if y[k] == 1:
                ub = min(ub, yG)
            else:
                lb = max(lb, yG)
        else:
            nfree += 1
            sf += yG
    rho = sf / nfree if nfree else (ub + lb) / 2
    out = np.zeros(l)
    out[aset] = alpha
    return out, rho, it, nshr, stopped


# ---- problems -------------------------------------------------------------------------------------------------------------------
def sym_gram(X, kind, gamma=None):
    """float64 kernel matrix of the rows, bit-exactly symmetric (the upper triangle mirrored), as rml_gram's matrices are"""
    X64 = np.asarray(X, dtype=np.float64)
    dot = X64 @ X64.T
    dot = np.triu(dot) + np.triu(dot, 1).T
    if kind == "linear":
        return dot
    sq = np.diag(dot).copy()
    return np.exp(-gamma * (sq[:, None] + sq[None, :] - 2.0 * dot))


REAL_KERNELS = [("linear", None, 0.01), ("linear", None, 10.0), ("rbf", 0.001, 100.0), ("rbf", 1.0, 10.0)]      # kind, gamma, C


def _problem(name, K, rows, n_pos, Cp, Cn, C, class_weight):
    return {"name": name, "K": K, "rows": np.asarray(rows, dtype=np.int32), "n_pos": int(n_pos), "Cp": float(Cp), "Cn": float(Cn),
            "C": C, "class_weight": class_weight}


@functools.lru_cache(maxsize=None)
def real_problems():
    """the three class pairs of the real XY rows (118, 395, 469 rows) x REAL_KERNELS, class_weight='balanced'"""
    X, y = G.real_xy()
    out = []
    for kind, gamma, C in REAL_KERNELS:
        K = sym_gram(X, kind, gamma)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ra, rb = np.nonzero(y == a)[0], np.nonzero(y == b)[0]
            n = len(ra) + len(rb)
            # compute_class_weight('balanced'): n / (2 * count), times C (libsvm's weighted_C)
            out.append(_problem("xy-%s-%s-C%s-%d%d" % (kind, gamma, C, a, b), K, np.concatenate([ra, rb]), len(ra),
                                C * (n / (2.0 * len(ra))), C * (n / (2.0 * len(rb))), C, "balanced"))
    return out


@functools.lru_cache(maxsize=None)
def big_problems():
    """N = 2 400 > 1 000 rows: libsvm's shrink counter is min(l, 1000), not l"""
    rng = np.random.default_rng(7)
    N, D = 2400, 48
    y = np.arange(N) % 2
    g = rng.standard_normal(D)
    X = (0.5 + 0.04 * (2 * y - 1)[:, None] * g[None, :] + 0.25 * rng.standard_normal((N, D))).astype(np.float32)
    ra, rb = np.nonzero(y == 0)[0], np.nonzero(y == 1)[0]
    rows = np.concatenate([ra, rb])
    return [_problem("big-linear-C1", sym_gram(X, "linear"), rows, len(ra), 1.0, 1.0, 1.0, None),
            _problem("big-rbf-0.5-C10", sym_gram(X, "rbf", 0.5), rows, len(ra), 10.0, 10.0, 10.0, None)]


@functools.lru_cache(maxsize=None)
def degenerate_problems():
    """twelve rows = four copies each of three vectors, alternating labels (quad_coef = 0: the TAU branch; 6 iterations), and two
    rows, one per class (1 iteration)"""
    V = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.25], [0.5, 0.5, 1.0]], dtype=np.float32)
    X = V[np.arange(12) % 3]
    y = np.arange(12) % 2
    ra, rb = np.nonzero(y == 0)[0], np.nonzero(y == 1)[0]
    X2 = np.array([[1.0, 0.0], [0.0, 1.0]], dtype=np.float32)
    return [_problem("copies-12", sym_gram(X, "linear"), np.concatenate([ra, rb]), len(ra), 1.0, 1.0, 1.0, None),
            _problem("two-rows", sym_gram(X2, "linear"), [0, 1], 1, 1.0, 1.0, 1.0, None)]


_SK = {}


def sklearn_fit(prob, shrinking=True, max_iter=-1):
    """SVC(kernel='precomputed') run live on the problem's sub-matrix in libsvm's row order; memoised.
    Returns (n_iter, support positions, alpha (= |dual_coef_| at the support positions, 0 elsewhere), |intercept_|)."""
    import warnings
    from sklearn.svm import SVC
    key = (prob["name"], shrinking, max_iter)
    if key not in _SK:
        rows = prob["rows"]
        Ks = np.ascontiguousarray(prob["K"][np.ix_(rows, rows)])
        lab = np.where(np.arange(len(rows)) < prob["n_pos"], 0, 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")             # ConvergenceWarning of the max_iter cases
            m = SVC(kernel="precomputed", C=prob["C"], class_weight=prob["class_weight"], shrinking=shrinking, max_iter=max_iter).fit(Ks, lab)
        a = np.zeros(len(rows))
        a[m.support_] = np.abs(m.dual_coef_[0])
        _SK[key] = (int(m.n_iter_[0]), np.sort(m.support_), a, abs(float(m.intercept_[0])))
    return _SK[key]


def check_against_sklearn(prob, alpha, rho, n_iter, shrinking=True, max_iter=-1):
    """the issue's equality criteria: n_iter, the support set, alpha bit-equal to |dual_coef_|, rho to intercept_ up to scikit-learn's
    sign flip of binary models"""
    it, sup, a, b = sklearn_fit(prob, shrinking, max_iter)
    name = prob["name"]
    assert int(n_iter) == it, (name, int(n_iter), it)
    assert np.array_equal(np.nonzero(alpha > 0)[0], sup), name
    assert np.array_equal(alpha, a), (name, np.abs(alpha - a).max())
    assert abs(float(rho)) == b, (name, float(rho), b)


def twin_solve(prob, eps=1e-3, shrinking=True, max_iter=-1):
    rows = prob["rows"]
    Ks = np.ascontiguousarray(prob["K"][np.ix_(rows, rows)])
    l = len(rows)
    ys = np.where(np.arange(l) < prob["n_pos"], 1, -1)
    return solve(Ks, ys, np.where(ys == 1, prob["Cp"], prob["Cn"]), eps, shrinking, max_iter)


# ---- the device interface on the host: plans of radar_ml_amd.train ----------------------------------------------------------------
def make_plan(T, probs, shrinking=True, max_iter=-1, eps=1e-3):
    """a radar_ml_amd.train plan (solve only: no fits) of problems that each bring their own matrix (problems address rows by
    index, so matrices of different sizes share one zero-padded stack); returns (matrices, plan)"""
    mats, recs, rows = [], [], []
    n = 0
    nmax = max(p["K"].shape[0] for p in probs)          # smaller matrices are zero-padded to the largest: one (nk, N, N) stack
    for p in probs:
        k = next((i for i, m in enumerate(mats) if m is p["K"]), None)
        if k is None:
            mats.append(p["K"])
            k = len(mats) - 1
        recs.append((k, len(p["rows"]), p["n_pos"], int(shrinking), max_iter, 0, n, n, p["Cp"], p["Cn"], eps))
        rows.append(p["rows"])
        n += len(p["rows"])
    plan = {"problems": np.array(recs, dtype=T.SMO_PROBLEM), "rows": np.concatenate(rows).astype(np.int32),
            "fits": np.zeros(0, dtype=T.SMO_FIT), "test_rows": np.zeros(0, np.int32), "test_y": np.zeros(0, np.int32), "n_classes": 2}
    stack = np.zeros((len(mats), nmax, nmax))
    for k, m in enumerate(mats):
        stack[k, :m.shape[0], :m.shape[0]] = m
    return stack, plan


def split_alpha(plan, alpha):
    return [alpha[int(r["alpha_off"]):int(r["alpha_off"]) + int(r["l"])] for r in plan["problems"]]


def twin_smo(X, kernels, plan, device=None):
    """NumPy twin of radar_ml_amd.train._smo (test oracle only): numpy_gram's matrices made symmetric, ``solve`` per problem,
    libsvm's decision values and vote per fit"""
    mats = [np.triu(K) + np.triu(K, 1).T for K in G.numpy_gram(X, kernels)]
    probs, rows = plan["problems"], plan["rows"]
    C = int(plan["n_classes"])
    P = C * (C - 1) // 2
    n_alpha = int((probs["alpha_off"] + probs["l"]).max()) if len(probs) else 0
    alpha, rho = np.zeros(n_alpha), np.zeros(len(probs))
    n_iter, stopped = np.zeros(len(probs), np.int32), np.zeros(len(probs), np.int32)
    for i, r in enumerate(probs):
        rr = rows[int(r["rows_off"]):int(r["rows_off"]) + int(r["l"])]
        Ks = np.ascontiguousarray(mats[int(r["matrix"])][np.ix_(rr, rr)])
        ys = np.where(np.arange(int(r["l"])) < int(r["n_pos"]), 1, -1)
        a, rho[i], n_iter[i], _, stp = solve(Ks, ys, np.where(ys == 1, r["Cp"], r["Cn"]), float(r["eps"]), bool(r["shrinking"]),
                                             int(r["max_iter"]))
        alpha[int(r["alpha_off"]):int(r["alpha_off"]) + int(r["l"])] = a
        stopped[i] = stp
    n_test = len(plan["test_rows"])
    dec, labels = np.zeros((n_test, P)), np.zeros(n_test, np.int32)
    correct = np.zeros(len(plan["fits"]), np.int32)
    pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
    for f, F in enumerate(plan["fits"]):
        sl = slice(int(F["test_off"]), int(F["test_off"]) + int(F["n_test"]))
        te = plan["test_rows"][sl]
        votes = np.zeros((len(te), C), np.int64)
        for p, (a, b) in enumerate(pairs):
            r = probs[int(F["prob0"]) + p]
            rr = rows[int(r["rows_off"]):int(r["rows_off"]) + int(r["l"])]
            al = alpha[int(r["alpha_off"]):int(r["alpha_off"]) + int(r["l"])]
            coef = np.where(np.arange(len(rr)) < int(r["n_pos"]), al, -al)
            Kt = mats[int(r["matrix"])][np.ix_(te, rr)]
            s = np.zeros(len(te))
            for k in np.nonzero(al > 0)[0]:             # libsvm's order: one add per support vector
                s += coef[k] * Kt[:, k]
            dec[sl, p] = s - rho[int(F["prob0"]) + p]
            votes[np.arange(len(te)), np.where(dec[sl, p] > 0, a, b)] += 1
        labels[sl] = votes.argmax(1)                    # the first maximum wins
        correct[f] = int((labels[sl] == plan["test_y"][sl]).sum())
    return {"alpha": alpha, "rho": rho, "n_iter": n_iter, "stopped": stopped, "dec": dec, "labels": labels, "correct": correct,
            "solve_s": 1e-3, "score_s": 1e-3, "matrix": lambda k: mats[k]}
