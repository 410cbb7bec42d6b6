"""Exact ties and exact saturation for the finish kernels of csrc/svm_finish.h (k_svm_finish, k_pairwise_proba, k_linear), with LIVE
scikit-learn as the reference (NumPy and scikit-learn only; tests/test_svm_ties_cpu.py checks the fixtures, tests/test_svm_ties_gpu.py
runs them on the device).

The geometry sweep (svm_geometry_common.py) keeps away from ties on purpose; here every decision value is exact in ANY arithmetic and
ANY summation order, so that the only thing a comparison can catch is the RULE applied at an equality:

  support vectors  one-hot rows, sv[m] = e_m with value 1.0 (code 255 on the c / 255 grid), ``per`` of them per class;
  weights          dual_coef and intercept are dyadic: multiples of 1/16 in [-1, 1], and +-2^-30 (all multiples of 2^-30 with
                   sum |.| < 2^6: 36 bits, exact in float64 whatever the order; the rows whose sums also fit the 24 bits of float32
                   are marked ``f32_ok`` -- computed per row, see _f32_safe);
  linear kernel    binary rows: K[n, m] = x_n[m] in {0, 1}; on the int8 path K = (65025 k) * (1 / 65025), exactly k for k = 0 and 1
                   (not for k = 3: the reason the SVs are one-hot), so dec[n, p] = sum_{m on} W[p, m] + b[p];
  RBF kernel       gamma = 1000; rows are the zero row, the SVs and one-hot rows off the SVs: a squared distance is 0 (K = 1) or
                   >= 1 (exp(<= -1000) underflows to 0 in libm and in rml_exp_neg), so dec[n, p] = W[p, m] + b[p] or b[p];
  null model       dual coefficients all zero: dec = intercept for ANY row on any kernel and path.

An RBF model has M + 1 distinct decision rows, each touching the pairs of ONE class: the full pattern list is asserted on the linear
fixture of every C, and a reduced list (RBF_PATTERNS) on the RBF one.

A vote in which all classes tie needs C (C - 1) / 2 pairs shared equally among C classes: odd C only (C = 3, 5); ``required(C, ..)``
says which patterns a C can hold.

pr > 1 (the ``1 + 1e-5`` clamp of sk:calibration.py "minimally exceeds 1.0") cannot be reached, by either finish kernel: for C > 2,
pr[c] / den with den = fl(pr[0] + .. + pr[C-1]) and every term >= 0: rounding is monotone, so den >= pr[c] and the correctly rounded
quotient is <= 1; for C = 2, pr[0] = fl(1 - pr[1]) with pr[1] in [0, 1].  The clamp is dead code on both sides; no row can show it.
"""
import functools
import types
import warnings

import numpy as np

import oracle_np as O
import svm_geometry_common as G

TINY = 2.0 ** -30
STEP = 1.0 / 16.0
GAMMA = 1000.0
GAP = 1e-6                       # no calibrated top-2 gap of a fixture row lies in (0, GAP)
CONTROL_GAP = 1e-3
PATHS = ("auto", "i8", "digits", "f64", "f32")
CLASS_COUNTS = (2, 3, 4, 5, 6)
KERNELS = ("linear", "rbf")
N_BATCH = 300
EDGE_POSITIONS = (0, 63, 64, 127, 128, 129, 255, 256, N_BATCH - 1)
LINEAR_D = (1, 63, 64, 65, 129)


# ---- the finish, restated in NumPy row by row (with the mutations the suite has to notice) ------------------------------------------------
MUTATIONS = ("vote_ge", "ovr_le", "vote_last_max", "proba_last_max", "no_uniform", "no_clamp", "invalid_not_marked")
PAIRWISE_MUTATIONS = ("no_clip", "iter_cap")
LINEAR_MUTATIONS = ("bin_score_ge", "bin_proba_ge", "label_last_max", "proba_last_max", "no_uniform", "no_clamp")
UNREACHABLE = ("no_clamp",)      # see the module docstring


def _expit(x):
    if x >= 0.0:
        return 1.0 / (1.0 + np.exp(-x))
    e = np.exp(x)
    return e / (1.0 + e)


def _argmax(v, last):
    b = 0
    for c in range(1, len(v)):
        if (v[c] >= v[b]) if last else (v[c] > v[b]):
            b = c
    return b


def _calibrate(T, a, b, C, mut):
    """the calibrated tail both k_svm_finish and k_linear end in"""
    with np.errstate(all="ignore"):
        if C == 2:
            p1 = _expit(-(a[0] * T[0] + b[0]))
            pr = [1.0 - p1, p1]
        else:
            pr = [_expit(-(a[c] * T[c] + b[c])) for c in range(C)]
            den = 0.0
            for v in pr:
                den += v
            if mut == "no_uniform":
                pr = [np.float64(v) / np.float64(den) for v in pr]
            else:
                pr = [v / den if den != 0.0 else 1.0 / C for v in pr]
        if mut != "no_clamp":
            pr = [1.0 if 1.0 < v <= 1.0 + 1e-5 else v for v in pr]
    return pr, _argmax(pr, mut == "proba_last_max")


def finish_np(dec, C, calib_a, calib_b, flags=None, mut=None):
    """k_svm_finish after the partial sums: vote, one-vs-rest values, calibration -- one row at a time, the kernel's operations in the
    kernel's order.  ``flags``: the forced-i8 validity of a row (0: invalid)."""
    dec = np.asarray(dec, dtype=np.float64)
    N, P = dec.shape
    out = types.SimpleNamespace(dec_ovo=dec.copy(), dec_ovr=np.zeros(N if C == 2 else (N, C)), proba=np.zeros((N, C)),
                                label_vote=np.zeros(N, np.int64), label_calib=np.zeros(N, np.int64))
    for n in range(N):
        d = dec[n]
        if flags is not None and not flags[n]:
            marked = mut != "invalid_not_marked"
            out.dec_ovo[n], out.dec_ovr[n], out.proba[n] = np.nan, np.nan, np.nan
            out.label_vote[n] = out.label_calib[n] = -1 if marked else 0
            continue
        vote = [0] * C
        p = 0
        for i in range(C):
            for j in range(i + 1, C):
                if (d[p] >= 0) if mut == "vote_ge" else (d[p] > 0):
                    vote[i] += 1
                else:
                    vote[j] += 1
                p += 1
        out.label_vote[n] = _argmax(vote, mut == "vote_last_max")
        if C == 2:
            T = [-d[0]]
            out.dec_ovr[n] = T[0]
        else:
            soc, vt = [0.0] * C, [0.0] * C
            p = 0
            for i in range(C):
                for j in range(i + 1, C):
                    conf = -d[p]
                    soc[i] -= conf
                    soc[j] += conf
                    if (d[p] <= 0) if mut == "ovr_le" else (d[p] < 0):
                        vt[j] += 1.0
                    else:
                        vt[i] += 1.0
                    p += 1
            T = [vt[c] + soc[c] / (3.0 * (abs(soc[c]) + 1.0)) for c in range(C)]
            out.dec_ovr[n] = T
        out.proba[n], out.label_calib[n] = _calibrate(T, calib_a, calib_b, C, mut)
    return out


def linear_np(X, coef, intercept, C, calib_a, calib_b, mut=None):
    """k_linear: scores, label, calibrated tail (binary: one score row, class 1)"""
    s = np.asarray(X, dtype=np.float64) @ np.asarray(coef, dtype=np.float64).T + np.asarray(intercept, dtype=np.float64)
    N = len(s)
    out = types.SimpleNamespace(dec=s[:, 0].copy() if C == 2 else s.copy(), label=np.zeros(N, np.int64), proba=np.zeros((N, C)),
                                label_calib=np.zeros(N, np.int64))
    for n in range(N):
        if C == 2:
            out.label[n] = int((s[n, 0] >= 0) if mut == "bin_score_ge" else (s[n, 0] > 0))
            pr, _ = _calibrate([s[n, 0]], calib_a, calib_b, 2, mut)
            out.proba[n] = pr
            out.label_calib[n] = int((pr[1] >= pr[0]) if mut == "bin_proba_ge" else (pr[1] > pr[0]))
        else:
            out.label[n] = _argmax(s[n], mut == "label_last_max")
            out.proba[n], out.label_calib[n] = _calibrate(s[n], calib_a, calib_b, C, mut)
    return out


def pairwise_np(dec, probA, probB, k, mut=None, cap=None):
    """k_pairwise_proba (libsvm's sigmoid_predict + multiclass_probability); returns (proba, iterations run per row: the cap when the
    loop never met its stopping rule)"""
    dec = np.asarray(dec, dtype=np.float64).reshape(len(dec), -1)
    N = len(dec)
    out, iters = np.empty((N, k)), np.zeros(N, np.int64)
    max_iter = max(100, k) if cap is None else cap
    if mut == "iter_cap":
        max_iter //= 2
    for n in range(N):
        r = np.zeros((k, k))
        q = 0
        for i in range(k):
            for j in range(i + 1, k):
                f = dec[n, q] * probA[q] + probB[q]
                s = np.exp(-f) / (1.0 + np.exp(-f)) if f >= 0 else 1.0 / (1.0 + np.exp(f))
                if mut != "no_clip":
                    s = min(max(s, 1e-7), 1 - 1e-7)
                r[i, j], r[j, i] = s, 1.0 - s
                q += 1
        p = np.full(k, 1.0 / k)
        Q = np.zeros((k, k))
        for t in range(k):
            for j in range(t):
                Q[t, t] += r[j, t] * r[j, t]
                Q[t, j] = Q[j, t]
            for j in range(t + 1, k):
                Q[t, t] += r[j, t] * r[j, t]
                Q[t, j] = -r[j, t] * r[t, j]
        eps = 0.005 / k
        it = 0
        with np.errstate(all="ignore"):
            while it < max_iter:
                Qp = Q @ p
                pQp = float(p @ Qp)
                if np.abs(Qp - pQp).max() < eps:
                    break
                for t in range(k):
                    diff = (-Qp[t] + pQp) / Q[t, t]
                    p[t] += diff
                    pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
                    Qp = (Qp + diff * Q[t]) / (1 + diff)
                    p = p / (1 + diff)
                it += 1
        out[n], iters[n] = p, it
    return out, iters


# ---- the dyadic menu ------------------------------------------------------------------------------------------------------------------------
def _menu(rng, shape, p_zero, p_tiny):
    v = rng.integers(-16, 17, shape) * STEP
    u = rng.random(shape)
    v = np.where(u < p_zero, 0.0, v)
    return np.where(u > 1.0 - p_tiny, rng.choice([-TINY, TINY], shape), v)


def _f32_safe(terms):
    """(N,) bool from (N, T) float64 terms of a sum: every partial sum, in any order, fits the 24 bits of a float32.  All non-zero
    terms are multiples of the smallest power of two g among them (dyadic menu), every partial sum is a multiple of g below
    sum |terms|: exact when sum |terms| / g < 2^24."""
    a = np.abs(terms)
    # the granularity of a dyadic a = k 2^-30: the lowest set bit of k
    k = np.rint(a * 2.0 ** 30).astype(np.int64)
    assert np.array_equal(k * TINY, a)
    low = np.where(k > 0, k & -k, np.int64(1) << 40)
    g = low.min(axis=1)
    return (k.sum(axis=1) // np.maximum(g, 1) < (1 << 24)) | (k.sum(axis=1) == 0)


# ---- patterns of a set of pair values --------------------------------------------------------------------------------------------------------
def votes_of(dec, C):
    v = np.zeros((len(dec), C), np.int64)
    p = 0
    for i in range(C):
        for j in range(i + 1, C):
            pos = dec[:, p] > 0
            v[pos, i] += 1
            v[~pos, j] += 1
            p += 1
    return v


def _top_gap(a):
    s = np.sort(a, axis=1)
    return s[:, -1] - s[:, -2]


def patterns_of(dec, C, calibs):
    """{name: (N,) bool} of the patterns a row of pair values holds, and ``between``: rows that are neither an exact tie nor separated"""
    N, P = dec.shape
    pat = {"zero_pair_%d" % p: dec[:, p] == 0.0 for p in range(P)}
    pat["tiny_pos"], pat["tiny_neg"] = (dec == TINY).any(1), (dec == -TINY).any(1)
    pat["step_pos"], pat["step_neg"] = (dec == STEP).any(1), (dec == -STEP).any(1)
    eq, un = calibs["equal"], calibs["unequal"]
    if C == 2:
        ovr = O.sklearn_decision_function(dec, C)
        gaps = [_top_gap(O.calibrated_proba(ovr, *cal)) for cal in (eq, un)]
        pat["proba_tie"] = gaps[0] == 0.0
    else:
        v = votes_of(dec, C)
        top = v == v.max(1, keepdims=True)
        many = top.sum(1) >= 2
        pat["vote_tie_all"] = top.all(1)
        pat["vote_cycle"] = top.all(1) & (dec != 0.0).all(1)
        pat["vote_tie_top_with_0"] = many & top[:, 0] & ~top.all(1)
        pat["vote_tie_top_without_0"] = many & ~top[:, 0]
        ovr = O.sklearn_decision_function(dec, C)
        tie = _top_gap(ovr) == 0.0
        gaps = [_top_gap(O.calibrated_proba(ovr, *cal)) for cal in (eq, un)]
        pat["ovr_tie"] = tie
        pat["proba_tie"] = tie & (gaps[0] == 0.0)
        pat["ovr_tie_unequal_calibrators"] = tie & (gaps[1] >= GAP)
    # a zero gap must come from a true tie (the same operations on the same bits), never from two different values rounding alike;
    # under unequal calibrators every row is separated
    true_tie = (dec[:, 0] == 0.0) if C == 2 else tie
    between = ((gaps[0] > 0) & (gaps[0] < GAP)) | (gaps[1] < GAP) | ((gaps[0] == 0.0) & ~true_tie)
    pat["control"] = (np.abs(dec) >= STEP).all(1) & (gaps[0] >= CONTROL_GAP) & (gaps[1] >= CONTROL_GAP)
    return pat, between


@functools.lru_cache(maxsize=None)
def reachable_vote_ties(C):
    """which vote-tie patterns ANY pair values of C classes can produce: every sign pattern of the C (C - 1) / 2 pairs, enumerated
    (an all-classes tie needs the pairs shared equally: odd C only; with three classes two tied classes at the top tie the third)"""
    P = C * (C - 1) // 2
    signs = ((np.arange(1 << P)[:, None] >> np.arange(P)) & 1) * 2.0 - 1.0
    v = votes_of(signs, C)
    top = v == v.max(1, keepdims=True)
    many = top.sum(1) >= 2
    found = {"vote_tie_all": top.all(1).any(), "vote_tie_top_with_0": (many & top[:, 0] & ~top.all(1)).any(),
             "vote_tie_top_without_0": (many & ~top[:, 0]).any()}
    found["vote_cycle"] = found["vote_tie_all"]
    return tuple(sorted(k for k, ok in found.items() if ok))


def required(C, kernel):
    """the patterns a fixture of C classes must hold, with the minimum row count of each"""
    P = C * (C - 1) // 2
    ties = reachable_vote_ties(C) if C >= 3 else ()
    if kernel == "rbf":
        need = {"zero_pair_%d" % p: 1 for p in range(P)}
        need.update(tiny_pos=1, tiny_neg=1, step_pos=1, step_neg=1, control=2)
        need.update({k: 1 for k in ties if k.startswith("vote_tie_top")})
        return need
    need = {"zero_pair_%d" % p: 2 for p in range(P)}
    need.update(tiny_pos=2, tiny_neg=2, step_pos=2, step_neg=2, proba_tie=2, control=20)
    need.update({k: 2 for k in ties})
    if C >= 3:
        need.update(ovr_tie=2, ovr_tie_unequal_calibrators=2)
    return need


RBF_PATTERNS = "zero pair in every position, +-2^-30, +-1/16, a top vote tie with and without class 0, controls"


# ---- the SVC fixture -------------------------------------------------------------------------------------------------------------------------
def _calibrators(C):
    """equal: one (a, b) for every class -- tied one-vs-rest values give bit-equal probabilities (b = 0 for two classes: T = -0.0 gives
    (0.5, 0.5)); unequal: the control; sat0 / sat1: a T + b beyond +-745 for every T in [-1/3, C - 2/3], every sigmoid exactly 0 / 1"""
    if C == 2:
        # a pair value of 2^-30 is to be a SEPARATED row (top-2 gap >= GAP): a = -4096 gives p1 - p0 ~ 2^-19; 1/16 already saturates
        return {"equal": (np.array([-4096.0]), np.array([0.0])), "unequal": (np.array([-4096.0]), np.array([0.125])),
                "sat0": (np.array([1.0]), np.array([800.0])), "sat1": (np.array([1.0]), np.array([-800.0]))}
    n = C
    # gentle slopes: T spans [-1/3, C - 2/3], and a steeper sigmoid saturates the top two of six classes to within 1e-3
    return {"equal": (np.full(n, -0.5), np.full(n, 0.25)),
            "unequal": (-0.5 - 0.0625 * np.arange(n), 0.125 + 0.0625 * np.arange(n)),
            "sat0": (np.full(n, 1.0), np.full(n, 800.0)),
            "sat1": (np.full(n, 1.0), np.full(n, -800.0))}


def _platt(C):
    """libsvm's own pair sigmoids: pair 0 steep (|dec A + B| > 17 from |dec| >= 9/16 on: the 1e-7 clip, both ends), the rest moderate"""
    P = C * (C - 1) // 2
    A = np.full(P, -4.0)
    A[0] = -32.0
    return A, 0.25 * (np.arange(P) % 3 - 1)


def _model(rng, C, kernel, D, per):
    M = per * C
    assert D >= M + 4 and M <= 18
    codes = np.zeros((M, D), np.uint8)
    codes[np.arange(M), np.arange(M)] = 255
    P = C * (C - 1) // 2
    dual = _menu(rng, (C - 1, M), 0.3, 0.08)
    # an RBF row sees ONE SV: dec = b + W[:, m], and SV m of class c reaches the pairs of c alone.  b is separated (|b| >= 1/8);
    # the first SV of a class cancels b on its pairs (zeros), the next ones land +-2^-30 and +-1/16 beside zero, the rest is
    # drawn.  The linear fixture has the same SVs (its one-hot rows are the RBF rows) and sums of them besides
    icpt = rng.integers(2, 17, P) * STEP * rng.choice([-1.0, 1.0], P)
    pair = {}
    for i in range(C):
        for j in range(i + 1, C):
            pair[i, j] = pair[j, i] = len(pair) // 2
    offs = (TINY, -TINY, STEP, -STEP)
    for c in range(C):
        for k in range(per):
            if k >= 3 or (k == per - 1 and c % 2 == 1):
                continue
            for o in range(C):
                if o != c:
                    row = o - 1 if o > c else o             # the dual_coef row that meets class o (oracle_np.ovo_weight_matrix)
                    q = pair[c, o]
                    dual[row, c * per + k] = -icpt[q] + (0.0 if k == 0 else offs[(c + q + 2 * (k - 1)) % 4])
    m = dict(codes=codes, sv=G.on_grid(codes).astype(np.float64), n_support=np.full(C, per, np.int32), dual_coef=dual, intercept=icpt,
             classes=np.arange(C), kernel=kernel, gamma=GAMMA)
    m["calibs"] = _calibrators(C)
    m["calib_a"], m["calib_b"] = m["calibs"]["equal"]
    m["probA"], m["probB"] = _platt(C)
    return m


def design_K(model, codes):
    """the kernel values of code rows against the one-hot SVs, by the construction (not by a kernel formula): linear x_n[m]; RBF 1
    where the row IS the SV, else 0"""
    M = len(model["codes"])
    on = (codes == 255).astype(np.float64)
    assert ((codes == 0) | (codes == 255)).all()
    if model["kernel"] == "linear":
        return on[:, :M]
    assert (on.sum(1) <= 1).all()
    return on[:, :M].copy()


def design_dec(model, codes):
    W = O.ovo_weight_matrix(model["dual_coef"], model["n_support"])
    return design_K(model, codes) @ W.T + model["intercept"]


def _candidates(rng, model, n):
    M, D = model["codes"].shape
    if model["kernel"] == "rbf":
        rows = np.zeros((1 + D, D), np.uint8)                    # the zero row, the SVs, one-hot rows off the SVs
        rows[1 + np.arange(D), np.arange(D)] = 255
        return rows
    on = rng.random((n, D)) < rng.uniform(0.05, 0.7, (n, 1))
    on[0], on[1] = False, True
    on[2:2 + D] = np.eye(D, dtype=bool)                          # the rows of the RBF design
    return (on * 255).astype(np.uint8)


def select_rows(pat, keep, everything=False, per_pattern=6, controls=40):
    """indices of the rows a fixture keeps: up to ``per_pattern`` rows of every pattern, at least ``controls`` control rows (as many as
    there are edge rows), edge rows and controls interleaved; ``everything``: all rows that are not in between (the RBF design has
    few)"""
    chosen, seen = [], set()

    def take(idx):
        for i in idx:
            if int(i) not in seen:
                seen.add(int(i))
                chosen.append(int(i))
    for name in sorted(pat):
        if name != "control":
            take(np.flatnonzero(pat[name] & keep)[:per_pattern])
    edge_n = len(chosen)
    take(np.flatnonzero(pat["control"] & keep)[:max(controls, edge_n)])
    if everything:
        take(np.flatnonzero(keep))
    e, c = chosen[:edge_n], chosen[edge_n:]
    mixed = []
    while e or c:
        if e:
            mixed.append(e.pop(0))
        if c:
            mixed.append(c.pop(0))
    return np.array(mixed)


class Fixture:
    """model (the dict shape of svm_geometry_common.make_model, plus ``calibs``, ``probA``, ``probB``), ``codes`` (N, D) uint8, ``X`` the
    on-grid float32 rows, ``dec`` the designed pair values (float64), ``pat`` the pattern masks, ``edge`` rows holding a tie or a zero,
    ``f32_ok`` rows whose sums fit float32."""

    def __init__(self, C, kernel, D, per, seed):
        self.C, self.kernel, self.D, self.seed = C, kernel, D, seed
        rng = np.random.default_rng([seed, C, KERNELS.index(kernel), D])
        self.model = m = _model(rng, C, kernel, D, per)
        cand = _candidates(rng, m, 8000)
        dec = design_dec(m, cand)
        pat, between = patterns_of(dec, C, m["calibs"])
        keep = ~between
        need = required(C, kernel)
        self.short = {k: (int((pat[k] & keep).sum()), v) for k, v in need.items() if (pat[k] & keep).sum() < v}
        idx = select_rows(pat, keep, everything=kernel == "rbf")
        self.codes = cand[idx]
        self.X = G.on_grid(self.codes)
        self.dec = dec[idx]
        self.pat = {k: v[idx] for k, v in pat.items()}
        self.between = between[idx]
        self.edge = np.zeros(len(idx), bool)
        for k, v in self.pat.items():
            if k != "control":
                self.edge |= v
        self.N = len(idx)
        W = O.ovo_weight_matrix(m["dual_coef"], m["n_support"])
        K = design_K(m, self.codes)
        terms = np.concatenate([K[:, None, :] * W[None, :, :], np.broadcast_to(m["intercept"][None, :, None], (self.N, len(W), 1))], axis=2)
        self.f32_ok = np.array([_f32_safe(terms[n]).all() for n in range(self.N)])

    def batch(self):
        """indices (N_BATCH,) into the fixture rows: edge rows at EDGE_POSITIONS, every row of the fixture at least once where it fits,
        controls between"""
        edge, rest = np.flatnonzero(self.edge), np.flatnonzero(~self.edge)
        if not len(rest):
            rest = edge
        idx = np.empty(N_BATCH, np.int64)
        allrows = np.arange(self.N)
        idx[:] = allrows[np.arange(N_BATCH) % self.N]
        for k, pos in enumerate(EDGE_POSITIONS):
            idx[pos] = edge[k % len(edge)]
            for nb in (pos - 1, pos + 1):
                if 0 <= nb < N_BATCH and nb not in EDGE_POSITIONS:
                    idx[nb] = rest[k % len(rest)]
        return idx

    def __repr__(self):
        return "ties-C%d-%s-D%d" % (self.C, self.kernel, self.D)


# seeds searched once on the CPU so that every required pattern is present (tests/test_svm_ties_cpu.py asserts it; a seed that fails
# there is replaced here, the requirement never)
SEEDS = {(5, "rbf", 20): 6, (5, "rbf", 32): 1, (6, "rbf", 23): 2, (6, "rbf", 32): 1}


@functools.lru_cache(maxsize=None)
def fixture(C, kernel, D=None):
    per = min(18 // C, 4) if kernel == "rbf" else 18 // C
    if D is None:
        D = per * C + 5
    per = min(per, (D - 4) // C)
    return Fixture(C, kernel, D, per, SEEDS.get((C, kernel, D), 0))


def null_model(C, kernel, D=37, M=11):
    """dual coefficients all zero: dec = intercept for any row"""
    m = G.make_model(3, M, D, C, "balanced", kernel)
    m["dual_coef"] = np.zeros_like(m["dual_coef"])
    m["calibs"] = _calibrators(C)
    rng = np.random.default_rng([C, 5])
    while True:                                     # every row has these pair values: they must not lie in between either
        m["intercept"] = _menu(rng, C * (C - 1) // 2, 0.4, 0.1)
        m["intercept"][0] = 0.0
        if not patterns_of(m["intercept"][None, :], C, m["calibs"])[1].any():
            break
    m["calib_a"], m["calib_b"] = m["calibs"]["equal"]
    m["probA"], m["probB"] = _platt(C)
    return m


# ---- volumes for the fused front doors -------------------------------------------------------------------------------------------------------
GRID = (4, 4, 8)
VOLUME_D = {"linear": 80, "rbf": 32}
VOLUME_MASK = {"linear": (True, True, True), "rbf": (True, False, False)}       # RBF: the xz plane alone -- one voxel, one feature


def volume_codes(vol, mode, ijk, mask):
    """the code rows of uint8 volumes by the CPU oracle's projection (xz | yz | xy, C order)"""
    B = len(vol)
    if mode == "max":
        planes = O.project_max(vol)
    else:
        per = [O.project_slice(vol[b], *ijk[b]) for b in range(B)]
        planes = [np.stack([q[i] for q in per]) for i in range(3)]
    return np.concatenate([p.reshape(B, -1) for p, keep in zip(planes, mask) if keep], axis=1).astype(np.uint8)


class VolumeFixture:
    """voxels 0 or 255 on a 4 x 4 x 8 grid, so the scaled features are 0 or 1: the model of fixture(C, kernel, VOLUME_D[kernel]), the
    frames chosen (by computing them) to hold its patterns.  ``mode``: "max" or "slice" (with ``ijk``)."""

    def __init__(self, C, kernel, mode):
        X, Y, Z = GRID
        self.C, self.kernel, self.mode, self.mask = C, kernel, mode, VOLUME_MASK[kernel]
        base = fixture(C, kernel, VOLUME_D[kernel])
        self.model = m = base.model
        rng = np.random.default_rng([C, KERNELS.index(kernel), mode == "max", 21])
        if kernel == "rbf":
            # one voxel (x, y, z) lights feature x * Z + z of the xz plane, whatever y is (slices are taken at j = y)
            B = base.N
            vol = np.zeros((B, X, Y, Z), np.uint8)
            ijk = np.stack([rng.integers(0, X, B), np.arange(B) % Y, rng.integers(0, Z, B)], axis=1)
            for b in range(B):
                on = np.flatnonzero(base.codes[b])
                if len(on):
                    vol[b, on[0] // Z, ijk[b, 1], on[0] % Z] = 255
        else:
            B = 4000
            vol = ((rng.random((B, X, Y, Z)) < rng.uniform(0.01, 0.25 if mode == "max" else 0.6, (B, 1, 1, 1))) * 255).astype(np.uint8)
            ijk = np.stack([rng.integers(0, n, B) for n in GRID], axis=1)
        codes = volume_codes(vol, mode, ijk, self.mask)
        if kernel == "rbf":
            assert np.array_equal(codes, base.codes)
            idx = np.arange(B)
        else:
            pat, between = patterns_of(design_dec(m, codes), C, m["calibs"])
            idx = select_rows(pat, ~between)
        self.vol, self.ijk, self.codes = vol[idx], ijk[idx].astype(np.int32), codes[idx]
        self.X = G.on_grid(self.codes)
        self.dec = design_dec(m, self.codes)
        self.pat, self.between = patterns_of(self.dec, C, m["calibs"])
        self.N = len(idx)

    def __repr__(self):
        return "ties-volumes-C%d-%s-%s" % (self.C, self.kernel, self.mode)


@functools.lru_cache(maxsize=None)
def volume_fixture(C, kernel, mode):
    return VolumeFixture(C, kernel, mode)


# ---- the k_linear fixture --------------------------------------------------------------------------------------------------------------------
class LinearFixture:
    def __init__(self, C, D, seed=0):
        self.C, self.D = C, D
        rng = np.random.default_rng([seed, C, D, 9])
        rows = 1 if C == 2 else C
        self.coef = _menu(rng, (rows, D), 0.3, 0.0)
        self.intercept = _menu(rng, rows, 0.0, 0.0)
        if D == 1:
            # two distinct rows (x = 0, 1): score 0 at x = 0 for the binary case; a top tie with class 0 at x = 0, without at x = 1
            self.coef[:, 0] = [0.5] if C == 2 else ([-1.0, 0.25, 0.25] + [0.0] * (C - 3))
            self.intercept[:] = [0.0] if C == 2 else ([0.5, 0.5, 0.5] + [-0.25] * (C - 3))
        self.calibs = _calibrators(C)
        n = 4000 if D > 1 else 2
        on = rng.random((n, D)) < rng.uniform(0.02, 0.5, (n, 1))
        on[0] = False
        on[1] = True
        s = on.astype(np.float64) @ self.coef.T + self.intercept
        pat = {"zero_score": (s == 0.0).any(1)}
        if C == 2:
            gaps = [_top_gap(O.calibrated_proba(s[:, 0], *self.calibs[k])) for k in ("equal", "unequal")]
            pat["proba_tie"] = gaps[0] == 0.0
            pat["control"] = (np.abs(s[:, 0]) >= STEP) & (gaps[0] >= CONTROL_GAP)
            between = ((gaps[0] > 0) & (gaps[0] < GAP)) | (gaps[1] < GAP) | ((gaps[0] == 0.0) & (s[:, 0] != 0.0))
        else:
            top = s == s.max(1, keepdims=True)
            many = top.sum(1) >= 2
            gaps = [_top_gap(O.calibrated_proba(s, *self.calibs[k])) for k in ("equal", "unequal")]
            pat["top_tie_with_0"] = many & top[:, 0]
            pat["top_tie_without_0"] = many & ~top[:, 0]
            pat["proba_tie"] = many & (gaps[0] == 0.0)
            pat["control"] = (_top_gap(s) >= STEP) & (gaps[0] >= CONTROL_GAP) & (gaps[1] >= CONTROL_GAP)
            between = ((gaps[0] > 0) & (gaps[0] < GAP)) | (gaps[1] < GAP) | ((gaps[0] == 0.0) & ~many)
        keep = ~between
        chosen, seen = [], set()
        for name in sorted(pat):
            lim = 8 if name != "control" else 60
            for i in np.flatnonzero(pat[name] & keep)[:lim]:
                if int(i) not in seen:
                    seen.add(int(i))
                    chosen.append(int(i))
        idx = np.array(sorted(chosen))
        self.X = on[idx].astype(np.float32)
        self.scores = s[idx]
        self.pat = {k: v[idx] for k, v in pat.items()}
        self.between = between[idx]
        self.N = len(idx)

    def need(self):
        if self.D == 1:
            return dict(zero_score=1, proba_tie=1) if self.C == 2 else dict(top_tie_with_0=1, top_tie_without_0=1, proba_tie=1)
        base = dict(zero_score=2, proba_tie=2, control=10)
        if self.C >= 3:
            base.update(top_tie_with_0=2, top_tie_without_0=2)
        return base

    def __repr__(self):
        return "ties-linear-C%d-D%d" % (self.C, self.D)


LINEAR_SEEDS = {(5, "rbf", 20): 6, (5, "rbf", 32): 1, (6, "rbf", 23): 2, (6, "rbf", 32): 1}


@functools.lru_cache(maxsize=None)
def linear_fixture(C, D):
    return LinearFixture(C, D, LINEAR_SEEDS.get((C, D), 0))


# ---- live scikit-learn references (never stored arrays) -----------------------------------------------------------------------------------
def live_svc(model, shape="ovr"):
    """an SVC fitted on anything of the right shape, then given the model: support_vectors_, _dual_coef_, _intercept_, _n_support,
    _gamma, _probA, _probB (private attributes of scikit-learn's libsvm wrapper; an ImportError or AttributeError here is a reason to
    skip the reference, never to replace it)"""
    from sklearn.svm import SVC
    C = len(model["classes"])
    M, D = model["sv"].shape
    Xf = np.zeros((2 * C, D))
    Xf[np.arange(2 * C), np.arange(2 * C) % D] = 1.0 + np.arange(2 * C)
    svc = SVC(kernel=model["kernel"], gamma=1.0, decision_function_shape=shape).fit(Xf, np.repeat(np.arange(C), 2))
    for name in ("support_", "support_vectors_", "_n_support", "_dual_coef_", "_intercept_", "_gamma", "_probA", "_probB"):
        if not hasattr(svc, name):
            raise AttributeError("this scikit-learn's SVC has no %s" % name)
    svc.support_ = np.arange(M, dtype=np.int32)
    svc.support_vectors_ = np.ascontiguousarray(model["sv"], dtype=np.float64)
    svc._n_support = np.asarray(model["n_support"], dtype=np.int32)
    svc._dual_coef_ = svc.dual_coef_ = np.ascontiguousarray(model["dual_coef"], dtype=np.float64)
    svc._intercept_ = svc.intercept_ = np.ascontiguousarray(model["intercept"], dtype=np.float64)
    svc._gamma = float(model["gamma"])
    svc.probability = True
    svc._probA = np.ascontiguousarray(model["probA"], dtype=np.float64)
    svc._probB = np.ascontiguousarray(model["probB"], dtype=np.float64)
    return svc


def live_calibrated(estimator, C, calib_a, calib_b):
    from sklearn.calibration import _CalibratedClassifier, _SigmoidCalibration
    cals = []
    for a, b in zip(calib_a, calib_b):
        c = _SigmoidCalibration()
        c.a_, c.b_ = float(a), float(b)
        cals.append(c)
    return _CalibratedClassifier(estimator, cals, classes=np.arange(C), method="sigmoid")


def live_sgd(coef, intercept, C):
    from sklearn.linear_model import SGDClassifier
    sgd = SGDClassifier()
    sgd.coef_ = np.ascontiguousarray(coef, dtype=np.float64)
    sgd.intercept_ = np.ascontiguousarray(intercept, dtype=np.float64)
    sgd.classes_ = np.arange(C)
    sgd.n_features_in_ = sgd.coef_.shape[1]
    return sgd


def svc_reference(model, X, calib="equal", proba=True):
    """what live scikit-learn says about float32 rows X: dec_ovo, dec_ovr, label_vote, the calibrated proba / label_calib under the
    named calibrators, and the bare SVC's predict_proba (pairwise)"""
    C = len(model["classes"])
    X = np.ascontiguousarray(X, dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ovr = live_svc(model, "ovr")
        ovo = live_svc(model, "ovo")
        dec_ovo = ovo.decision_function(X).reshape(len(X), -1)
        if C == 2:
            dec_ovo = -dec_ovo                                  # sk:svm/_base.py: the public binary value is -dec of libsvm
        a, b = model["calibs"][calib]
        p = live_calibrated(ovr, C, a, b).predict_proba(X)
        ref = types.SimpleNamespace(dec_ovo=dec_ovo, dec_ovr=ovr.decision_function(X), label_vote=ovr.predict(X), proba=p,
                                    label_calib=p.argmax(axis=1))
        if proba:
            ref.pairwise = ovr.predict_proba(X)
    return ref


def linear_reference(fx, calib="equal"):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sgd = live_sgd(fx.coef, fx.intercept, fx.C)
        a, b = fx.calibs[calib]
        p = live_calibrated(sgd, fx.C, a, b).predict_proba(fx.X)
        return types.SimpleNamespace(dec=sgd.decision_function(fx.X), label=sgd.predict(fx.X), proba=p, label_calib=p.argmax(axis=1))
