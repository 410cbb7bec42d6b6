"""Synthetic SVC models, sample rows and two float64 references for the geometry sweep of csrc/svm.hip (NumPy only).

The golden models pin the arithmetic to scikit-learn at four feature lengths; this module makes models of ANY (M, D, C) without a fit,
so that tests/test_svm_geometry_gpu.py can walk the tile, K-step, batch and pair-count edges of the kernels one axis at a time, and
tests/test_svm_geometry_cpu.py can check -- without a GPU -- that the generated cases are fit to judge a kernel (no near-ties, a spread
of kernel values, the two references agreeing to the input-rounding floor).

Two references:
  ref_exact    integer code distances (int64) / 255^2, float64 exp, K @ W.T + intercept: no input rounding at all -- the yardstick of the
               exact (int8) routes, which compute the same integers;
  ref_f32rows  oracle_np.svm_decision_ovo on the float32 rows, i.e. float32(c / 255) inputs as libsvm sees them -- the yardstick of the
               float routes (f64, f32, digits), which read those float32 values.
"""
import functools
import types

import numpy as np

import oracle_np as O

F255 = np.float32(255.0)
OFF_GRID = np.float32(0.9990234375)       # rows * OFF_GRID leave the code grid (the factor test_svm_gpu.py uses)
NEAR_TIE = 1e-6                           # a |pair value| or a top-2 probability gap below this is a near-tie
CAP_MARGIN = 1e-5                         # the widest label margin (10 x the bar of a route) at which the 1 % cap on excluded rows is asserted
PATHS = ("auto", "i8", "f64", "f32", "digits")


# ---- generator ---------------------------------------------------------------------------------------------------------------------------
def draw_codes(rng, shape):
    """uint8 codes, uniform 0..255 with half the entries zeroed (radar rows are sparse)"""
    c = rng.integers(0, 256, shape)
    c[rng.random(shape) < 0.5] = 0
    return c.astype(np.uint8)


def _balanced(M, C):
    return [M // C + (1 if c < M % C else 0) for c in range(C)]


def pattern_allowed(M, C, pattern):
    if pattern == "balanced":
        return M >= 1
    if pattern == "single":
        return M >= C                      # one SV in class 0 and at least one in every other class
    if pattern == "empty":
        return C >= 3 and M >= C - 1
    return False


def n_support_of(M, C, pattern):
    """balanced: M split as evenly as possible (M < C leaves the last classes empty); single: class 0 holds exactly one SV, the rest is
    balanced (a class block ends inside the first tile); empty: the last class holds no SV (rml_svm_load documents n_support >= 0)."""
    assert pattern_allowed(M, C, pattern), (M, C, pattern)
    if pattern == "balanced":
        ns = _balanced(M, C)
    elif pattern == "single":
        ns = [1] + _balanced(M - 1, C - 1)
    else:
        ns = _balanced(M, C - 1) + [0]
    assert sum(ns) == M and len(ns) == C
    return np.array(ns, dtype=np.int32)


def make_rows(rng, codes, N):
    """N code rows: row n is a copy of a random SV with a per-row fraction f_n ~ U[0, 0.6] of its entries redrawn, so that the kernel
    values against the source SV span roughly (0.37, 1] instead of clustering; row 0 IS SV 0 (K = 1 exactly)."""
    M, D = codes.shape
    src = rng.integers(0, M, N)
    rows = codes[src].copy()
    frac = rng.uniform(0.0, 0.6, N)
    redraw = rng.random((N, D)) < frac[:, None]
    fresh = draw_codes(rng, (N, D))
    rows[redraw] = fresh[redraw]
    rows[0] = codes[0]
    return rows


def code_sq_distances(rows, codes):
    """integer squared code distances (N, M), int64: |x|^2 + |s|^2 - 2 x.s in integers (no rounding anywhere)"""
    x = rows.astype(np.int64)
    s = codes.astype(np.int64)
    return (x * x).sum(1)[:, None] + (s * s).sum(1)[None, :] - 2 * (x @ s.T)


def gamma_for(rows, codes):
    """65025 / median(non-zero integer squared code distance rows <-> SVs): the median kernel value is e^-1.  1.0 when every distance
    is 0 (D = 1 with one code)."""
    d2 = code_sq_distances(rows, codes)
    nz = d2[d2 > 0]
    return float(65025.0 / np.median(nz)) if nz.size else 1.0


def on_grid(codes):
    """the float32 rows of integer codes: float32(c) / float32(255), as the reference scales its features (train.py:667)"""
    return codes.astype(np.float32) / F255


def make_model(seed, M, D, C, pattern="balanced", kernel="rbf"):
    """What rml.GpuSVC takes (plus ``codes``, the uint8 SV codes), with no scikit-learn fit: SVs on the code grid and
    float32-representable (as conftest.svm_model_arrays makes them), |dual_coef| <= 1 so that sum |w| <= M, calibrators that exercise
    proba / label_calib.  gamma comes from a probe batch of 64 rows drawn by make_rows from the model's own generator, so the model does
    not depend on the batch it is later asked about (the N axis runs ONE model against batches of every size)."""
    rng = np.random.default_rng([int(seed), M, D, C, PATTERNS.index(pattern), KERNELS.index(kernel)])
    codes = draw_codes(rng, (M, D))
    P = C * (C - 1) // 2
    ncal = 1 if C == 2 else C
    m = dict(codes=codes, sv=on_grid(codes).astype(np.float64), n_support=n_support_of(M, C, pattern),
             dual_coef=rng.uniform(-1.0, 1.0, (C - 1, M)), intercept=rng.uniform(-0.5, 0.5, P),
             calib_a=rng.uniform(-3.0, -0.5, ncal), calib_b=rng.uniform(-0.5, 0.5, ncal),
             classes=np.arange(C), kernel=kernel)
    m["gamma"] = gamma_for(make_rows(rng, codes, 64), codes)
    return m


PATTERNS = ("balanced", "single", "empty")
KERNELS = ("rbf", "linear")


# ---- references --------------------------------------------------------------------------------------------------------------------------
def _tails(model, dec, K):
    """vote / ovr / calibration tails of oracle_np on pair values ``dec`` (N, P)"""
    C = len(model["classes"])
    ovr = O.sklearn_decision_function(dec, C)                       # (N,) = -dec for two classes, like SVC.decision_function
    proba = O.calibrated_proba(ovr, model["calib_a"], model["calib_b"])
    return types.SimpleNamespace(K=K, dec_ovo=dec, dec_ovr=ovr, proba=proba, label_vote=O.svm_vote_labels(dec, C),
                                 label_calib=O.calibrated_labels(proba))


def ref_exact(model, row_codes):
    """int64 code distances (int64 dot products for the linear kernel) / 255^2, float64 exp, K @ W.T + intercept"""
    if model["kernel"] == "linear":
        K = (row_codes.astype(np.int64) @ model["codes"].astype(np.int64).T) / 65025.0
    else:
        K = np.exp(-model["gamma"] * (code_sq_distances(row_codes, model["codes"]) / 65025.0))
    W = O.ovo_weight_matrix(model["dual_coef"], model["n_support"])
    return _tails(model, K @ W.T + model["intercept"], K)


def ref_f32rows(model, X):
    """oracle_np.svm_decision_ovo on the float32 rows X: what the float paths see"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    K = O.svm_kernel_values(X, model["sv"], model["gamma"], model["kernel"])
    dec = O.svm_decision_ovo(X, model["sv"], model["dual_coef"], model["intercept"], model["n_support"], model["gamma"], model["kernel"])
    return _tails(model, dec, K)


def margins(ref):
    """per row: the smallest |pair value| (what the vote hangs on) and the calibrated top-2 probability gap"""
    pair = np.abs(ref.dec_ovo).min(axis=1)
    top = np.sort(ref.proba, axis=1)
    return pair, top[:, -1] - top[:, -2]


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One (M, D, C, N, pattern, kernel): model, code rows, float rows on and off the grid, and the references (computed once, on first
    use, and never written to: every test that needs them shares them)."""

    def __init__(self, M, D, C, N, pattern="balanced", kernel="rbf", seed=0):
        self.key = (M, D, C, N, pattern, kernel, seed)
        self.M, self.D, self.C, self.N, self.pattern, self.kernel = M, D, C, N, pattern, kernel
        self.model = make_model(seed, M, D, C, pattern, kernel)
        rng = np.random.default_rng([int(seed), M, D, C, N, 77])
        self.codes = make_rows(rng, self.model["codes"], N)
        self.X = on_grid(self.codes)
        self.Xoff = self.X * OFF_GRID

    @functools.cached_property
    def exact(self):
        return ref_exact(self.model, self.codes)

    @functools.cached_property
    def f32(self):
        return ref_f32rows(self.model, self.X)

    @functools.cached_property
    def f32off(self):
        return ref_f32rows(self.model, self.Xoff)

    def first(self, n):
        """the first n rows of this case as a case of its own (rows are independent: the references are slices)"""
        return _Head(self, n)

    def __repr__(self):
        return "M%d-D%d-C%d-N%d-%s-%s" % (self.M, self.D, self.C, self.N, self.pattern, self.kernel)


def _cut(ref, n):
    return types.SimpleNamespace(**{k: v[:n] for k, v in vars(ref).items()})


class _Head:
    def __init__(self, whole, n):
        assert 1 <= n <= whole.N
        self.whole, self.N = whole, n
        self.M, self.D, self.C, self.pattern, self.kernel, self.model = whole.M, whole.D, whole.C, whole.pattern, whole.kernel, whole.model
        self.codes, self.X, self.Xoff = whole.codes[:n], whole.X[:n], whole.Xoff[:n]

    exact = property(lambda self: _cut(self.whole.exact, self.N))
    f32 = property(lambda self: _cut(self.whole.f32, self.N))
    f32off = property(lambda self: _cut(self.whole.f32off, self.N))

    def __repr__(self):
        return "%r[:%d]" % (self.whole, self.N)


# a case whose seed-0 draw breaks the near-tie cap of tests/test_svm_geometry_cpu.py gets another seed here (never a wider cap).
# (128, 896, 6, 128, single): with six classes two calibrated sigmoids can both saturate (|a| T up to 15: 1 - 3e-7), and seed 0 drew
# eight rows whose top-2 probabilities were that close
SEEDS = {(128, 896, 6, 128, "single", "rbf"): 1}


@functools.lru_cache(maxsize=None)
def case(M, D, C, N, pattern="balanced", kernel="rbf"):
    return Case(M, D, C, N, pattern, kernel, SEEDS.get((M, D, C, N, pattern, kernel), 0))


# ---- the star design: one axis at a time around (M=129, D=129, N=129, C=3, balanced, rbf) --------------------------------------------------
BASE = dict(M=129, D=129, N=129, C=3)
M_AXIS = (1, 2, 7, 8, 9, 127, 128, 129, 255, 256, 257, 385)
D_AXIS = (1, 3, 31, 32, 33, 127, 128, 129, 255, 257, 896, 897, 1025, 1153, 1409)      # KT = 1, 2, 3, 7, 8, 9, 10, 12
N_AXIS = (1, 2, 3, 4, 5, 8, 9, 127, 128, 129, 255, 256, 257, 300, 513)
N_AXIS_D = (129, 1025)                     # the tile GEMM, and split-K (KT = 9)
N_MAX = max(N_AXIS)
C_AXIS = tuple((C, p) for C in (2, 3, 4, 5, 6) for p in ("balanced", "single")) + ((3, "empty"),)
RING_N, RING_M, RING_D, RING_C = (256, 257, 513), (129, 257), (1, 129, 300, 513, 640, 1025), (2, 3, 4)     # KT = 1, 2, 3, 5, 5, 9


def ring_cases():
    """every value of the four axes of the forced ring kernel in eight runs (KT on both sides of the five ring slots, ragged N and M)"""
    out = []
    for i, D in enumerate(RING_D):
        out.append((RING_M[i % 2], D, RING_C[i % 3], RING_N[i % 3]))
    out += [(257, 129, 2, 513), (129, 1025, 4, 257)]
    return out


# (M, D, C, N, pattern): hand-picked corners
CORNERS = ((1, 1, 2, 1, "balanced"), (385, 1409, 6, 513, "balanced"), (257, 1025, 3, 300, "single"), (8, 1024, 3, 8, "balanced"),
           (7, 1025, 4, 9, "single"), (129, 897, 5, 8, "single"), (2, 3, 2, 257, "single"), (256, 128, 3, 256, "empty"),
           (128, 896, 6, 128, "single"), (385, 33, 4, 5, "empty"), (9, 1153, 2, 129, "balanced"), (255, 257, 5, 255, "balanced"))


def all_case_keys():
    """(M, D, C, N, pattern, kernel) of everything tests/test_svm_geometry_gpu.py parametrises; the N axis as (.., N_MAX, ..) once per D,
    its smaller batches being the first rows of that one"""
    b = BASE
    keys = []
    for kernel in KERNELS:
        keys += [(M, b["D"], b["C"], b["N"], "balanced", kernel) for M in M_AXIS]
        keys += [(b["M"], D, b["C"], b["N"], "balanced", kernel) for D in D_AXIS]
    keys += [(b["M"], D, b["C"], N_MAX, "balanced", "rbf") for D in N_AXIS_D]
    keys += [(b["M"], b["D"], C, b["N"], p, "rbf") for C, p in C_AXIS]
    keys += [(M, D, C, N, p, "rbf") for M, D, C, N, p in CORNERS]
    keys += [(M, D, C, N, "balanced", "rbf") for M, D, C, N in ring_cases()]
    keys += [(M, D, 3, N, "balanced", "rbf") for M, D, N in KMAT_SHAPES]
    seen, out = set(), []
    for k in keys:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


KMAT_SHAPES = ((1, 1, 1), (129, 129, 129), (257, 1025, 300))        # (M, D, N) of the rml_svm_kernel_matrix checks
# ... and of its float64 route at the other pair counts: kernel values only, no label is judged, so these are not among all_case_keys
KMAT_F64_SHAPE, KMAT_F64_C = (129, 33, 129), (2, 4, 5, 6)
