"""Float64 twins, derived error bounds and the case table for csrc/convt_train.hip (NumPy only; shared by test_convt_train_cpu.py,
which shows that twins and cases are fit to judge a kernel, and test_convt_train_gpu.py, which judges the kernels).

Layout: X (N, H, W, 128), W (ci, 4, 4, co) -- the channels_last storage of torch's ConvTranspose2d weight --, Z and dZ (N, 2H, 2W, 128);
input pixel (iy, ix) meets output pixel (2 iy + ky - 1, 2 ix + kx - 1) through tap (ky, kx), and what falls outside a plane is
dropped.  Every twin takes inputs that were already rounded to the half type and widened to float64; nothing inside a twin is rounded.

Bounds: conv_train_common.bound -- 0.5 ulp_half(|ref| + s) + s + smallest subnormal, s = 4 n u sum |terms|, u = 2^-24 (half products
are exact in float32; first order, hence the 4).  n: forward 4 * 128 (2 x 2 taps meet an output pixel), data gradient 16 * 128, weight
gradient N H W -- or the longest chain of the kernel's own split where the caller passes it (nn_common.convt4s2_wgrad_chain).  Each
twin also returns the sum of |terms| (the twin of the absolute inputs)."""
import numpy as np

from bnact_common import round_half
from conv_train_common import bound, smallest_subnormal  # noqa: F401  (the bound is that module's, unchanged)

KINDS = ("float16", "bfloat16")
CH = 128
# constants of csrc/convt_train.hip (k_convt_ig: 32 pixels per wave, 8 waves; k_convt_wgrad and wgrad_plan)
TILE, BLOCK_PIXELS, CHP, PIECE_MIN, MAX_PIECES = 32, 256, 64, 128, 64
TAPS = [(ky, kx) for ky in range(4) for kx in range(4)]
DROPPED_TAP = (1, 2)
MUTATIONS = ("drop_tap", "swap_phase_taps", "clamp_border_tap", "drop_last_pixel")


def wgrad_plan(pixels):
    """(pieces, pixels per piece): wgrad_plan of convt_train.hip"""
    n = min(max(-(-pixels // PIECE_MIN), 1), MAX_PIECES)
    ln = max(-(-(-(-pixels // n)) // CHP) * CHP, CHP)
    return -(-pixels // ln), ln


# ---- twins -----------------------------------------------------------------------------------------------------------------------------
def _pairs(k, n, clamp=None):
    """(input indices i, output indices o = 2 i + k - 1) that meet along one axis of n input pixels.  ``clamp``: the pair that falls
    outside is kept instead of dropped -- "in": the output border pixel reads the clamped input row (forward), "out": the input border
    pixel reads the clamped output row (gradients)."""
    i = np.arange(n)
    o = 2 * i + k - 1
    ok = (o >= 0) & (o < 2 * n)
    if clamp == "out":
        return i, np.clip(o, 0, 2 * n - 1)
    i, o = i[ok], o[ok]
    if clamp == "in":       # o = 0 with k = 3 asks for i = -1, o = 2n - 1 with k = 0 for i = n
        if k == 3:
            i, o = np.concatenate(([0], i)), np.concatenate(([0], o))
        if k == 0:
            i, o = np.concatenate((i, [n - 1])), np.concatenate((o, [2 * n - 1]))
    return i, o


def _taps(mutation):
    """(ky, kx, the ky whose weights are used)"""
    for ky, kx in TAPS:
        if mutation == "drop_tap" and (ky, kx) == DROPPED_TAP:
            continue
        yield ky, kx, (ky ^ 2 if mutation == "swap_phase_taps" else ky)


def _fwd(X, W, mutation):
    N, H, Wd, _ = X.shape
    Z = np.zeros((N, 2 * H, 2 * Wd, W.shape[3]))
    for ky, kx, kw in _taps(mutation):
        iy, oy = _pairs(ky, H, "in" if mutation == "clamp_border_tap" else None)
        ix, ox = _pairs(kx, Wd)
        Z[:, oy[:, None], ox[None, :]] += X[:, iy[:, None], ix[None, :]] @ W[:, kw, kx]
    if mutation == "drop_last_pixel":
        Z[-1, -1, -1] = 0.0
    return Z


def forward(X, W, mutation=None):
    """(Z, sum |terms|)"""
    return _fwd(X, W, mutation), _fwd(np.abs(X), np.abs(W), mutation)


def _dgrad(dZ, W, mutation):
    N, H2, W2, _ = dZ.shape
    H, Wd = H2 // 2, W2 // 2
    dX = np.zeros((N, H, Wd, W.shape[0]))
    for ky, kx, kw in _taps(mutation):
        iy, oy = _pairs(ky, H, "out" if mutation == "clamp_border_tap" else None)
        ix, ox = _pairs(kx, Wd)
        dX[:, iy[:, None], ix[None, :]] += dZ[:, oy[:, None], ox[None, :]] @ W[:, kw, kx].T
    if mutation == "drop_last_pixel":
        dX[-1, -1, -1] = 0.0
    return dX


def dgrad(dZ, W, mutation=None):
    """(dX, sum |terms|)"""
    return _dgrad(dZ, W, mutation), _dgrad(np.abs(dZ), np.abs(W), mutation)


def _wgrad(X, dZ, mutation):
    N, H, Wd, ci = X.shape
    co = dZ.shape[3]
    dW = np.zeros((ci, 4, 4, co))
    if mutation == "drop_last_pixel":
        X = X.copy()
        X[-1, -1, -1] = 0.0
    for ky, kx, kw in _taps(mutation):
        iy, oy = _pairs(ky, H, "out" if mutation == "clamp_border_tap" else None)
        ix, ox = _pairs(kx, Wd)
        dW[:, kw, kx] = X[:, iy[:, None], ix[None, :]].reshape(-1, ci).T @ dZ[:, oy[:, None], ox[None, :]].reshape(-1, co)
    return dW


def wgrad(X, dZ, mutation=None):
    """(dW, sum |terms|)"""
    return _wgrad(X, dZ, mutation), _wgrad(np.abs(X), np.abs(dZ), mutation)


def chains(c, wgrad_chain=None):
    """n of the three bounds for case c; wgrad_chain(pixels) tightens the weight gradient's"""
    P = c["N"] * c["H"] * c["W"]
    return dict(forward=4 * CH, dgrad=16 * CH, wgrad=wgrad_chain(P) if wgrad_chain else P)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _case(name, kind, N, H, W, sparse=False):
    return dict(name="%s-%s%s" % (name, "h" if kind == "float16" else "b", "-sparse" if sparse else ""), kind=kind, N=N, H=H, W=W,
                sparse=sparse, path=name)


SPLIT_PIXELS = 576          # 24 x 24: five pieces of 128 pixels, the last one 64


def cases():
    cs = []
    for kind in KINDS:
        cs.append(_case("one", kind, 1, 8, 8))                  # the smallest plane: every border rule at once
        for sparse in (False, True):
            cs.append(_case("seamx", kind, 3, 8, 16, sparse))   # tiles of two rows, a second workgroup that is half empty
        cs.append(_case("seamy", kind, 2, 16, 8))               # tiles of four rows
        cs.append(_case("three", kind, 2, 24, 8))               # non-square
        cs.append(_case("split", kind, 1, 24, 24))              # SPLIT_PIXELS
        cs.append(_case("big", kind, 4, 32, 32))                # 4096 pixels
    for i, c in enumerate(cs):
        c["seed"] = 9500 + i
    return cs


def reaches(c):
    """does the case exercise what its row of the table is there for?"""
    N, H, W = c["N"], c["H"], c["W"]
    P = N * H * W
    pieces, ln = wgrad_plan(P)
    path = c["path"]
    if path == "one":       # one workgroup, one staged tile, and no pixel further than 3 from each of the four borders
        return N == 1 and H == 8 and W == 8 and P <= BLOCK_PIXELS and P == CHP and pieces == 1
    if path == "seamx":     # a 32-pixel tile spans rows along x, a sample spans tiles, the last workgroup has idle waves
        return W < TILE and TILE % W == 0 and W > H and N > 1 and P > BLOCK_PIXELS and P % BLOCK_PIXELS != 0 and pieces >= 2
    if path == "seamy":     # narrow and tall: a tile holds four rows
        return H > W and TILE // W >= 4 and N > 1
    if path == "three":     # non-square, H no power of two: tiles and samples end at different pixels
        return H != W and H % 16 != 0 and N > 1 and P > BLOCK_PIXELS
    if path == "split":     # rows that no tile boundary respects, pixels whose every tap is inside, >= 2 pieces and a shorter last one
        return (P == SPLIT_PIXELS and TILE % W != 0 and W % TILE != 0 and H > 2 and W > 2 and pieces >= 2 and P % ln != 0
                and P > BLOCK_PIXELS)
    if path == "big":
        return P == 4096 and P > 4 * BLOCK_PIXELS and pieces >= 2 and W == TILE
    return False


def make(c):
    """X, W, dZ: float64 arrays of half values, drawn as conv_train_common.make draws them"""
    rng = np.random.default_rng(c["seed"])
    N, H, W, kind = c["N"], c["H"], c["W"], c["kind"]
    X = rng.standard_normal((N, H, W, CH), dtype=np.float32)
    dZ = rng.standard_normal((N, 2 * H, 2 * W, CH), dtype=np.float32)
    if c["sparse"]:         # radar-like: the activation of the background per channel, 4 % returns
        back = rng.uniform(-0.3, 1.0, CH).astype(np.float32)
        X = np.where(rng.random((N, H, W, 1)) < 0.04, X, back)
        backz = rng.uniform(-1e-2, 1e-2, CH).astype(np.float32)
        dZ = np.where(rng.random((N, 2 * H, 2 * W, 1)) < 0.04, dZ, backz)
    Wt = rng.normal(0, 0.3, (CH, 4, 4, CH)).astype(np.float32)
    return dict(X=round_half(X, kind), W=round_half(Wt, kind), dZ=round_half(dZ, kind))
