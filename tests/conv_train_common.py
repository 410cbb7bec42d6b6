"""Float64 twins, derived error bounds and the case table for csrc/conv_train.hip (NumPy only; shared by test_conv_train_cpu.py,
which shows that twins and cases are fit to judge a kernel, and test_conv_train_gpu.py, which judges the kernels).

Layout: X (N, 2 Ho + 1, 2 Wo + 1, Cin) -- already padded --, W (Cout, 3, 3, Cin), Z and dZ (N, Ho, Wo, Cout).  Every twin takes inputs that
were already rounded to the half type and widened to float64; nothing inside a twin is rounded.

Bounds (u = 2^-24, the convention of bnact_common.py).  A product of two half values is exact in float32, so an output that is a sum
of n such products, added in float32 in ANY order and rounded to the half type once, is off by at most
    0.5 ulp_half(|ref| + s) + s + (smallest subnormal of the half type),   s = 4 n u sum |terms|
(first order, hence the 4; the ulp is taken at |ref| + s because the kernel rounds its own float32 value).  n: forward 9 Cin, data
gradient 4 Cout (the largest parity class), weight gradient N Ho Wo -- or the longest chain of the kernel's own split where the
caller passes it (nn_common.conv3s2_wgrad_chain).  Each twin also returns the sum of |terms| (the twin of the absolute inputs)."""
import numpy as np

from bnact_common import HALF, U, round_half, ulp_h

KINDS = ("float16", "bfloat16")
PAIRS = ((128, 64), (64, 32))
# constants of csrc/conv_train.hip (wgrad_plan, k_conv_ig, k_conv_wgrad)
TILE, BLOCK_PIXELS, CHP, PIECE_MIN, MAX_PIECES = 32, 128, 64, 256, 128
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]
DROPPED_TAP = (1, 2)


def wgrad_plan(pixels):
    """(pieces, pixels per piece): wgrad_plan of conv_train.hip"""
    n = min(max(-(-pixels // PIECE_MIN), 1), MAX_PIECES)
    ln = max(-(-(-(-pixels // n)) // CHP) * CHP, CHP)
    return -(-pixels // ln), ln


def smallest_subnormal(kind):
    p, emin = HALF[kind]
    return 2.0 ** (emin - p + 1)


# ---- twins -----------------------------------------------------------------------------------------------------------------------------
def _fwd(X, W, mutation):
    N, Hp, Wp, _ = X.shape
    Ho, Wo = (Hp - 1) // 2, (Wp - 1) // 2
    Z = np.zeros((N, Ho, Wo, W.shape[0]))
    for ky, kx in TAPS:
        if mutation == "drop_tap" and (ky, kx) == DROPPED_TAP:
            continue
        Z += X[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] @ W[:, ky, kx].T
    if mutation == "drop_last_pixel":
        Z[-1, -1, -1] = 0.0
    return Z


def forward(X, W, mutation=None):
    """(Z, sum |terms|)"""
    return _fwd(X, W, mutation), _fwd(np.abs(X), np.abs(W), mutation)


def _dgrad(dZ, W, mutation):
    N, Ho, Wo, _ = dZ.shape
    dX = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, W.shape[3]))
    for ky, kx in TAPS:
        if mutation == "drop_tap" and (ky, kx) == DROPPED_TAP:
            continue
        yw = {0: 1, 1: 0, 2: 2}[ky] if mutation == "parity_shift" else ky     # rows of the wrong parity class take the tap
        dX[:, yw:yw + 2 * Ho:2, kx:kx + 2 * Wo:2] += dZ @ W[:, ky, kx]
    if mutation == "keep_border_tap":       # the tap that falls outside dZ is read from the clamped row instead of being dropped
        for kx in range(3):
            dX[:, 0, kx:kx + 2 * Wo:2] += dZ[:, 0] @ W[:, 2, kx]
            dX[:, 2 * Ho, kx:kx + 2 * Wo:2] += dZ[:, Ho - 1] @ W[:, 0, kx]
    if mutation == "drop_last_pixel":
        dX[-1, -1, -1] = 0.0
    return dX


def dgrad(dZ, W, mutation=None):
    """(dX, the whole padded tensor; sum |terms|)"""
    return _dgrad(dZ, W, mutation), _dgrad(np.abs(dZ), np.abs(W), mutation)


def _wgrad(X, dZ, mutation):
    N, Ho, Wo, Cout = dZ.shape
    dW = np.zeros((Cout, 3, 3, X.shape[3]))
    g = dZ.reshape(-1, Cout)
    if mutation == "drop_last_pixel":
        g = g.copy()
        g[-1] = 0.0
    for ky, kx in TAPS:
        if mutation == "drop_tap" and (ky, kx) == DROPPED_TAP:
            continue
        dW[:, ky, kx] = g.T @ X[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2].reshape(g.shape[0], -1)
    return dW


def wgrad(X, dZ, mutation=None):
    """(dW, sum |terms|)"""
    return _wgrad(X, dZ, mutation), _wgrad(np.abs(X), np.abs(dZ), mutation)


MUTATIONS = {"forward": ("drop_tap", "drop_last_pixel"),
             "dgrad": ("drop_tap", "parity_shift", "drop_last_pixel", "keep_border_tap"),
             "wgrad": ("drop_tap", "drop_last_pixel")}


def bound(ref, abs_sum, n, kind):
    s = 4.0 * n * U * abs_sum
    return 0.5 * ulp_h(np.abs(ref) + s, kind) + s + smallest_subnormal(kind)


def chains(c, wgrad_chain=None):
    """n of the three bounds for case c; wgrad_chain(pixels, cin) tightens the weight gradient's"""
    P = c["N"] * c["Ho"] * c["Wo"]
    return dict(forward=9 * c["cin"], dgrad=4 * c["cout"], wgrad=wgrad_chain(P, c["cin"]) if wgrad_chain else P)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _case(name, kind, pair, N, Ho, Wo, sparse=False, path=None):
    return dict(name="%s-%d-%s%s" % (name, pair[0], "h" if kind == "float16" else "b", "-sparse" if sparse else ""), kind=kind, cin=pair[0],
                cout=pair[1], N=N, Ho=Ho, Wo=Wo, sparse=sparse, path=path or name)


SPLIT_PIXELS = 2 * PIECE_MIN + CHP // 2 + 8          # 552 = 23 x 24: three pieces of 192 pixels, the last one 168 = two tiles + 40


def cases():
    cs = []
    for kind in KINDS:
        for pair in PAIRS:
            cs.append(_case("one", kind, pair, 1, 1, 1))                    # one pixel: every border rule at once
            cs.append(_case("row", kind, pair, 2, 1, 5))
            cs.append(_case("col", kind, pair, 2, 5, 1))
            for sparse in (False, True):                                    # 105 pixels: a tail tile, tiles across rows and samples
                cs.append(_case("tail", kind, pair, 3, 5, 7, sparse))
            cs.append(_case("split", kind, pair, 1, 23, 24))                # SPLIT_PIXELS
        for sparse in (False, True):                                        # the net in miniature (16 x 16 planes)
            cs.append(_case("mini", kind, PAIRS[0], 2, 8, 8, sparse))
            cs.append(_case("mini", kind, PAIRS[1], 2, 4, 4, sparse))
        cs.append(_case("big", kind, PAIRS[1], 4, 32, 32))                  # 4096 pixels
    for i, c in enumerate(cs):
        c["seed"] = 9000 + i
    return cs


def reaches(c):
    """does the case exercise what its row of the table is there for?"""
    P = c["N"] * c["Ho"] * c["Wo"]
    pieces, ln = wgrad_plan(P)
    hw = c["Ho"] * c["Wo"]
    path = c["path"]
    if path == "one":
        return P == 1
    if path == "row":
        return c["Ho"] == 1 and c["Wo"] > 1
    if path == "col":
        return c["Wo"] == 1 and c["Ho"] > 1
    if path == "tail":      # a partial 32-pixel tile; 32-pixel tiles that cross a row and a sample; the same for the classes of dX
        return P % TILE != 0 and P > TILE and c["Wo"] < TILE and hw % TILE != 0 and c["N"] > 1 and P < CHP * 2 and P % CHP != 0
    if path == "mini":
        return (c["cin"], c["Ho"], c["Wo"]) in ((128, 8, 8), (64, 4, 4)) and c["N"] == 2
    if path == "big":
        return P == 4096 and P > BLOCK_PIXELS and pieces >= 2
    if path == "split":
        return P == SPLIT_PIXELS and pieces >= 2 and P % ln != 0 and (P % ln) % CHP != 0 and P > BLOCK_PIXELS
    return False


def make(c):
    """X (with non-zero values in its pad row and column: a kernel that skips them is caught), W, dZ: float64 arrays of half values"""
    rng = np.random.default_rng(c["seed"])
    N, Ho, Wo, cin, cout, kind = c["N"], c["Ho"], c["Wo"], c["cin"], c["cout"], c["kind"]
    X = rng.standard_normal((N, 2 * Ho + 1, 2 * Wo + 1, cin), dtype=np.float32)
    dZ = rng.standard_normal((N, Ho, Wo, cout), dtype=np.float32)
    if c["sparse"]:         # radar-like: the activation of the background per channel, 4 % returns
        back = rng.uniform(-0.3, 1.0, cin).astype(np.float32)
        X = np.where(rng.random((N, 2 * Ho + 1, 2 * Wo + 1, 1)) < 0.04, X, back)
        backz = rng.uniform(-1e-2, 1e-2, cout).astype(np.float32)
        dZ = np.where(rng.random((N, Ho, Wo, 1)) < 0.04, dZ, backz)
    W = rng.normal(0, 0.3, (cout, 3, 3, cin)).astype(np.float32)
    return dict(X=round_half(X, kind), W=round_half(W, kind), dZ=round_half(dZ, kind))
