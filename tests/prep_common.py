"""A NumPy twin of the data-set preparation of the two network trainers (dnn.py:185-277, sgan.py:617-727), written against the SciPy /
Pillow / scikit-learn calls those functions rest on: scaling, rotate / clipped zoom / noise with the clamp to [-1, 1], bicubic resize,
stack, shuffle, split, class balancing.  tests/golden/prep_golden.npz holds the inputs, every draw and the small arrays of the
reference's run in full and the large ones as SHA-256 digests of their bytes (nine samples at 128 x 128 x 3 do not fit a fixture):
test_prep_cpu.py shows that this twin reproduces all of them bit for bit, so the GPU tests compare the kernels with the twin's arrays.
"""
import collections
import hashlib

import numpy as np

SETTINGS = 2            # augmentation settings of the golden: 0 the defaults (1.0, 0.3, 1.0), 1 (15.0, 0.3, 0.05)
STAGES = ("rotate", "zoom", "noise")


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


class Args:
    def __init__(self, augment, train_split=0.8):
        self.augment, self.train_split = augment, train_split


def golden_dataset(g):
    """[(xz, yz, xy), ...] float32 planes in [0, 255], labels, supervised mask: six Walabot samples, then three small ones"""
    data = [tuple(g["w%d" % p][i] for p in range(3)) for i in range(len(g["w0"]))]
    data += [tuple(g["s%d" % p][i] for p in range(3)) for i in range(len(g["s0"]))]
    return data, [str(v) for v in g["labels"]], g["sup"].astype(bool)


# ---- the stages ---------------------------------------------------------------------------------------------------------------
def scale(p):
    return (np.asarray(p, np.float32) - np.float32(127.5)) / np.float32(127.5)


def clamp(p, lo=-1.0, hi=1.0):
    p = np.array(p, dtype=np.float32)
    p[p > hi] = hi
    p[p < lo] = lo
    return p


def rotate(p, angle):
    from scipy import ndimage
    return clamp(ndimage.rotate(np.asarray(p, np.float32), angle, reshape=False))


def clipped_zoom(p, f):
    from scipy import ndimage
    p = np.asarray(p, np.float32)
    H, W = p.shape
    if f == 1:
        return clamp(p)
    if f < 1:
        zh, zw = int(np.round(H * f)), int(np.round(W * f))
        out = np.zeros_like(p)
        t, l = (H - zh) // 2, (W - zw) // 2
        out[t:t + zh, l:l + zw] = ndimage.zoom(p, (f, f))
        return clamp(out)
    ch, cw = int(np.ceil(H / f)), int(np.ceil(W / f))
    t, l = (H - ch) // 2, (W - cw) // 2
    big = ndimage.zoom(p[t:t + ch, l:l + cw], (f, f))
    tt, tl = (big.shape[0] - H) // 2, (big.shape[1] - W) // 2
    return clamp(big[tt:tt + H, tl:tl + W])


def add_noise(p, draw):
    return clamp(np.asarray(p, np.float32) + np.float32(draw))


def resize(p, rescale):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(p, dtype=np.float32)).resize(tuple(rescale), resample=Image.BICUBIC))


def chain(p, angle=None, zoom=None, noise=None):
    """one scaled plane through the stages that are not None; returns the plane after each stage that ran, in order"""
    outs = []
    if angle is not None:
        p = rotate(p, angle)
        outs.append(p)
    if zoom is not None:
        p = clipped_zoom(p, zoom)
        outs.append(p)
    if noise is not None:
        p = add_noise(p, noise)
        outs.append(p)
    return outs


# ---- the data set -------------------------------------------------------------------------------------------------------------
def draws(n, nproj, setting, rng):
    """per sample: nproj angles and one factor from np.random.uniform, nproj noise draws from rng; a None range draws nothing"""
    rot, zr, sd = setting
    angles = np.full((n, nproj), np.nan)
    zoom = np.full((n,), np.nan)
    noise = np.full((n, nproj), np.nan)
    for i in range(n):
        if rot is not None:
            angles[i] = [np.random.uniform(-rot, rot) for _ in range(nproj)]
        if zr is not None:
            zoom[i] = np.random.uniform(1.0 - zr, 1.0 + zr)
        if sd is not None:
            noise[i] = [rng.normal(scale=sd) for _ in range(nproj)]
    return angles, zoom, noise


def balance_picks(y, rng):
    from sklearn.utils import resample
    mc = collections.Counter(int(v) for v in y).most_common()
    if len({c for _, c in mc}) == 1:
        return None
    picks = np.concatenate([resample(np.nonzero(y == cls)[0], replace=True, n_samples=mc[0][1], random_state=1234) for cls, _ in mc])
    idx = np.arange(len(picks))
    rng.shuffle(idx)
    return picks[idx]


def preprocess(args, data, labels, rescale, rng, samples_sup=None):
    """dict of everything ``preprocess_data`` returns or decides; with ``samples_sup`` the SGAN's variant (balanced training set)"""
    n = len(data)
    planes = [[scale(p) for p in s] for s in data]
    out = {}
    if args.augment:
        angles, zoom, noise = draws(n, 3, (1.0, 0.3, 1.0), rng)
        planes = [[chain(p, angles[i, k], zoom[i], noise[i, k])[-1] for k, p in enumerate(s)] for i, s in enumerate(planes)]
        out.update(angles=angles, zoom=zoom, noise=noise)
    classes, y = np.unique(np.asarray(labels), return_inverse=True)
    counts = np.bincount(y)
    out["w_keys"] = np.arange(len(classes))
    out["w_vals"] = np.array([round(float(counts.max()) / c, 2) for c in counts])
    X = np.stack([np.stack([resize(p, rescale) for p in s], axis=-1) for s in planes])
    order = np.arange(n)
    rng.shuffle(order)
    split = min(int(n * args.train_split), n)
    X, y = X[order], y[order]
    out.update(order=order, X_train=X[:split], y_train=y[:split], X_val=X[split:], y_val=y[split:], n_classes=len(classes))
    if samples_sup is not None:
        sup = np.asarray(samples_sup, bool)[order][:split]
        picks = balance_picks(y[:split], rng)
        out["sup_train"] = sup
        out["bal_idx"] = np.arange(split) if picks is None else picks
        out["X_bal"], out["y_bal"], out["sup_bal"] = out["X_train"][out["bal_idx"]], y[:split][out["bal_idx"]], sup[out["bal_idx"]]
        out["val_is_train"] = split == n
        if split == n:
            out["X_val"], out["y_val"] = out["X_train"], out["y_train"]
    return out


_CACHE = {}


def twin_runs():
    """The twin's arrays for the golden's inputs, computed once per session and left unchanged: ``stage[k][i][p]`` = [scaled, after rotate,
    after zoom, after noise] of setting k, sample i, projection p from the RECORDED draws; ``resized1[i][p]`` the 80 x 80 resize of setting
    1's final planes; ``runs[(module, augment)]`` = :func:`preprocess` with both random sources seeded as the golden's run was."""
    if _CACHE:
        return _CACHE
    from conftest import load_golden            # here, not at the top: tools/prep_bench.py --host times the functions above
    g = load_golden("prep_golden.npz")
    data, labels, sup = golden_dataset(g)
    stage = []
    for k in range(SETTINGS):
        stage.append([[[scale(p)] + chain(scale(p), g["angles%d" % k][i, pi], g["zoom%d" % k][i], g["noise%d" % k][i, pi])
                       for pi, p in enumerate(s)] for i, s in enumerate(data)])
    runs = {}
    for mod, rescale in (("dnn", (80, 80)), ("sgan", (128, 128))):
        for aug in (0, 1):
            np.random.seed(int(g["np_seed0"]))
            runs[(mod, aug)] = preprocess(Args(bool(aug)), data, labels, rescale, np.random.default_rng(1234), sup if mod == "sgan" else None)
    _CACHE.update(g=g, data=data, labels=labels, sup=sup, stage=stage, runs=runs,
                  resized1=[[resize(stage[1][i][pi][-1], (80, 80)) for pi in range(3)] for i in range(len(data))])
    return _CACHE
