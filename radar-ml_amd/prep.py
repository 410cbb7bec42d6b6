"""The data-set preparation in front of the two network trainers, ``preprocess_data`` of dnn.py:185-277 and sgan.py:617-727: the
[-1, 1] scaling, the optional ``augment_data`` chain (dnn.py:94-182; sgan.py:238-326 is the same function), Pillow's bicubic
resize, stack, shuffle, split and -- for the SGAN -- ``balance_classes`` (sgan.py:329-393).

The host does what depends on order and is tiny, the device does the arrays:

* :func:`plan_dataset` makes every random draw of the whole data set first, in the order the reference makes them sample by sample
  (per sample one ``np.random.uniform`` per projection for the angles, one for the zoom factor, one ``rng.normal`` per projection
  for the noise; then ``rng.shuffle`` of the index on the same generator; then the balance's resampling and shuffle), encodes the
  labels and works out the class weights.  It touches no GPU.
* :func:`run_plan` is one ``rml_augment_chain`` launch (csrc/augment_chain.hip) and one ``rml_resize_bicubic`` launch per
  (projection, plane shape) group, one gather for shuffle and split, one for the balanced training set.

``radar_ml_amd.dnn`` and ``radar_ml_amd.sgan`` hold the front doors with the reference's names.  Planes are handled in float32, as
everywhere in this tree: integer or float64 data-set planes are converted first (the reference would scale those in float64)."""
import collections

import numpy as np

from . import _lib
from .augment import rotation_params

RADAR_MAX = 255.0       # common.py RADAR_MAX
RANDOM_SEED = 1234      # dnn.py:29, sgan.py:35


def _torch():
    import torch
    return torch


class AugmentDraws:
    """The draws of ``augment_data`` for n samples of nproj projections: ``angles`` (n, nproj) degrees, ``zoom`` (n,) factors,
    ``noise`` (n, nproj); None where the stage is skipped (its range is None)."""

    def __init__(self, angles, zoom, noise):
        self.angles, self.zoom, self.noise = angles, zoom, noise

    @property
    def stages(self):
        return ((_lib.CHAIN_ROTATE if self.angles is not None else 0) | (_lib.CHAIN_ZOOM if self.zoom is not None else 0)
                | (_lib.CHAIN_NOISE if self.noise is not None else 0))

    def params(self, rows, pi, shape):
        """(len(rows), 8) float64 for ``rml_augment_chain``: the planes of projection ``pi`` (all of ``shape``) of the samples ``rows``"""
        par = np.zeros((len(rows), 8), np.float64)
        par[:, 6] = 1.0
        if self.angles is not None:
            par[:, :6] = [rotation_params(self.angles[r, pi], shape) for r in rows]
        if self.zoom is not None:
            par[:, 6] = self.zoom[rows]
        if self.noise is not None:
            par[:, 7] = self.noise[rows, pi]
        return par


def draw_augment(n, nproj, rotation_range, zoom_range, noise_sd, rng):
    """The draws ``[augment_data(d) for d in data]`` makes (dnn.py:209), in its order: per sample the angles (one ``np.random.uniform``
    per projection), the zoom factor (one ``np.random.uniform``), the noise (one ``rng.normal(scale=noise_sd)`` per projection).  A
    range that is None skips its stage and its draws."""
    angles = np.empty((n, nproj)) if rotation_range is not None else None
    zoom = np.empty((n,)) if zoom_range is not None else None
    noise = np.empty((n, nproj)) if noise_sd is not None else None
    for i in range(n):
        if angles is not None:
            for p in range(nproj):
                angles[i, p] = np.random.uniform(-1 * rotation_range, rotation_range)
        if zoom is not None:
            zoom[i] = np.random.uniform(1.0 - zoom_range, 1.0 + zoom_range)
        if noise is not None:
            for p in range(nproj):
                noise[i, p] = rng.normal(scale=noise_sd)
    return AugmentDraws(angles, zoom, noise)


def chain_planes(planes, stages, params=None, sub=0.0, div=0.0, lo=-1.0, hi=1.0, device=None):
    """One batch of equally shaped planes through ``rml_augment_chain``.  planes: (B,H,W) float32 (numpy or CUDA tensor); ``stages``: a
    mask of ``_lib.CHAIN_ROTATE | CHAIN_ZOOM | CHAIN_NOISE``; params: (B,8) float64 (see :meth:`AugmentDraws.params`).  Returns a CUDA
    float32 tensor (B,H,W)."""
    torch = _torch()
    lib = _lib.load()
    if isinstance(planes, torch.Tensor) and planes.is_cuda and device is None:
        dev = planes.device
    else:
        dev = _lib.device_of(device)
    src = planes if isinstance(planes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float32))
    src = src.to(device=dev, dtype=torch.float32).contiguous()
    if src.ndim != 3:
        raise ValueError("planes must be (B,H,W)")
    B, H, W = (int(v) for v in src.shape)
    par = None
    if stages:
        par = np.ascontiguousarray(params, dtype=np.float64)
        if par.shape != (B, 8):
            raise ValueError("params: (B, 8) expected, got %s" % (par.shape,))
        par = torch.from_numpy(par).to(dev)
    dst = torch.empty_like(src)
    with torch.cuda.device(dev):
        _lib.check(lib.rml_augment_chain(_lib.context(dev), int(stages), _lib.ptr(src), H * W, B, H, W, float(sub), float(div), float(lo),
                                         float(hi), _lib.ptr(par), _lib.ptr(dst), _lib.stream_ptr(dev)), "rml_augment_chain")
    return dst


def augment_data(x, rotation_range=1.0, zoom_range=0.3, noise_sd=1.0, rng=None, device=None):
    """``augment_data`` of dnn.py:94-182 for one sample: ``x`` is a tuple of projections already scaled to [-1, 1]; every projection is
    rotated by its own angle, all are zoomed by one factor, every one gets its own noise draw; each stage clamps to [-1, 1].  Same
    arguments and order of draws as the reference (see :func:`draw_augment`); ``rng`` is the generator of the noise.  Returns a tuple of
    float32 planes: NumPy arrays, or CUDA tensors where ``x`` held CUDA tensors."""
    torch = _torch()
    draws = draw_augment(1, len(x), rotation_range, zoom_range, noise_sd, rng)
    out = []
    for pi, p in enumerate(x):
        on_dev = isinstance(p, torch.Tensor) and p.is_cuda
        plane = p if isinstance(p, torch.Tensor) else np.asarray(p, dtype=np.float32)
        res = chain_planes(plane[None], draws.stages, draws.params([0], pi, tuple(plane.shape)), device=device)[0]
        out.append(res if on_dev else res.cpu().numpy())
    return tuple(out)


def encode_labels(labels):
    """``LabelEncoder().fit_transform(labels)`` and the class weights of dnn.py:213-220: (encoded labels, n_classes,
    {class: round(largest class size / class size, 2)})."""
    _, enc = np.unique(np.asarray(labels), return_inverse=True)
    enc = enc.reshape(-1)
    counter = collections.Counter(enc)
    max_v = float(max(counter.values()))
    return enc, len(counter), {cls: round(max_v / v, 2) for cls, v in counter.items()}


def balance_indices(labels, shuffle=True, rng=None):
    """The rows ``balance_classes`` (sgan.py:329-393) keeps, as indices into its input, or None when every class already has the same
    size: per class, from the most common down, ``sklearn.utils.resample(..., replace=True, n_samples=<largest class>,
    random_state=1234)``; then one ``rng.shuffle`` of the positions."""
    from sklearn import utils
    labels = np.asarray(labels)
    mc = collections.Counter(labels.tolist()).most_common()
    if len(set(c for _, c in mc)) == 1:
        return None
    majority = mc[0][1]
    picks = []
    for cls, _ in mc:
        rows = np.nonzero(labels == cls)[0]
        picks.append(utils.resample(rows, replace=True, n_samples=majority, random_state=RANDOM_SEED))
    picks = np.concatenate(picks)
    if shuffle:
        idx = np.arange(picks.size)
        rng.shuffle(idx)
        picks = picks[idx]
    return picks


def take_rows(a, rows):
    """a[rows] along axis 0: one device gather for a CUDA tensor, NumPy indexing otherwise"""
    torch = _torch()
    if isinstance(a, torch.Tensor):
        return a.index_select(0, torch.as_tensor(np.asarray(rows), dtype=torch.long, device=a.device))
    return np.asarray(a)[rows]


def balance_classes(data, labels, samples_sup, shuffle=True, rng=None):
    """``balance_classes`` of sgan.py:329-393: upsample every class to the size of the largest one.  ``data``: (N, ...) NumPy array or CUDA
    tensor (then the gather runs on the device and the result stays there); ``labels``, ``samples_sup``: (N,) host arrays.  Returns its
    three inputs themselves when the classes are balanced already."""
    picks = balance_indices(labels, shuffle, rng)
    if picks is None:
        return data, labels, samples_sup
    return take_rows(data, picks), np.asarray(labels)[picks], np.asarray(samples_sup)[picks]


class Plan:
    """What :func:`plan_dataset` decided on the host: ``draws`` (AugmentDraws or None), ``labels`` (encoded, data-set order), ``order``
    (the shuffled index), ``split``, ``n_classes``, ``w_classes``, ``sup`` (bool, data-set order, or None), ``balance`` (indices into
    the training part, or None: no SGAN balancing, or balanced already) and ``val_is_train`` (the SGAN's rule for an empty validation
    set: the validation set is the training part before balancing)."""


def plan_dataset(args, n, nproj, labels, rng, samples_sup=None, balance=False):
    """Every order-dependent decision of ``preprocess_data`` for n samples, in the reference's order on the reference's random sources:
    the augmentation draws of all samples (``args.augment``), ``rng.shuffle`` of the index, the split at ``int(n * args.train_split)``
    and, with ``balance``, the resampling of the training part."""
    if n < 1 or nproj < 1:
        raise ValueError("preprocess_data: an empty data set")
    plan = Plan()
    plan.draws = draw_augment(n, nproj, 1.0, 0.3, 1.0, rng) if args.augment else None       # the defaults of augment_data(d), dnn.py:209
    plan.labels, plan.n_classes, plan.w_classes = encode_labels(labels)
    if len(plan.labels) != n:
        raise ValueError("preprocess_data: %d labels for %d samples" % (len(plan.labels), n))
    plan.sup = None if samples_sup is None else np.array(samples_sup, dtype=bool)
    idx = np.arange(n)
    rng.shuffle(idx)
    plan.order = idx
    plan.split = min(int(n * args.train_split), n)
    plan.balance = balance_indices(plan.labels[idx][:plan.split], True, rng) if balance else None
    # sgan.py:722-723: an empty validation set is replaced by the training part as it was before balancing (dnn.py returns it empty)
    plan.val_is_train = bool(balance) and plan.split == n
    return plan


def device_samples(data, draws, rescale, device=None):
    """The array work in data-set order: (N, out_h, out_w, nproj) CUDA float32 from ``data`` = [(xz, yz, xy), ...] in [0, RADAR_MAX].  Per
    projection and plane shape (data sets may mix radar arenas) one ``rml_augment_chain`` launch (scaling included) and one
    ``rml_resize_bicubic`` launch, or the resize alone with its own scaling when ``draws`` is None."""
    torch = _torch()
    from .nn_common import resize_bicubic
    dev = _lib.device_of(device)
    n, nproj = len(data), len(data[0])
    out_hw = (int(rescale[1]), int(rescale[0]))             # Pillow's size is (width, height)
    half = RADAR_MAX / 2.0
    out = torch.empty((nproj, n) + out_hw, dtype=torch.float32, device=dev)
    for pi in range(nproj):
        groups = {}
        for i, s in enumerate(data):
            groups.setdefault(tuple(np.shape(s[pi])), []).append(i)
        for shape, rows in groups.items():
            if len(shape) != 2:
                raise ValueError("preprocess_data: projections are 2-D planes, got shape %s" % (shape,))
            planes = torch.from_numpy(np.stack([np.asarray(data[i][pi], dtype=np.float32) for i in rows])).to(dev)
            if draws is not None:
                planes = chain_planes(planes, draws.stages, draws.params(rows, pi, shape), sub=half, div=half)
            res = resize_bicubic(planes, out_hw, scale=draws is None)
            if len(rows) == n:
                out[pi] = res
            else:
                out[pi].index_copy_(0, torch.as_tensor(rows, dtype=torch.long, device=dev), res)
    return out.permute(1, 2, 3, 0)          # (N, out_h, out_w, nproj): a view, made dense by the gather of run_plan


def run_plan(plan, data, rescale, device=None):
    """The device half: returns (X_train, X_val, X_train_balanced or None) as CUDA float32 tensors (rows, out_h, out_w, nproj)."""
    torch = _torch()
    X = device_samples(data, plan.draws, rescale, device)
    X = X.index_select(0, torch.as_tensor(plan.order, dtype=torch.long, device=X.device))       # shuffle and split: one gather
    X_train, X_val = X[:plan.split], X[plan.split:]
    X_bal = take_rows(X_train, plan.balance) if plan.balance is not None else None
    return X_train, X_val, X_bal


def _host(t, return_numpy):
    return t.cpu().numpy() if return_numpy else t


def preprocess_dnn(args, data, labels, rescale, rng, device=None, return_numpy=True):
    """dnn.py:185-277; see ``radar_ml_amd.dnn.preprocess_data``."""
    plan = plan_dataset(args, len(data), len(data[0]) if len(data) else 0, labels, rng)         # raises on an empty data set
    X_train, X_val, _ = run_plan(plan, data, rescale, device)
    y = plan.labels[plan.order]
    return (_host(X_train, return_numpy), y[:plan.split], _host(X_val, return_numpy), y[plan.split:], plan.n_classes, plan.w_classes)


def preprocess_sgan(args, data, labels, samples_sup, rescale, rng, device=None, return_numpy=True):
    """sgan.py:617-727; see ``radar_ml_amd.sgan.preprocess_data``."""
    plan = plan_dataset(args, len(data), len(data[0]) if len(data) else 0, labels, rng, samples_sup=samples_sup, balance=True)
    X_train, X_val, X_bal = run_plan(plan, data, rescale, device)
    y, sup = plan.labels[plan.order], plan.sup[plan.order]
    y_train, sup_train = y[:plan.split], sup[:plan.split]
    if plan.balance is None:
        train_set = (_host(X_train, return_numpy), y_train, sup_train)
    else:
        train_set = (_host(X_bal, return_numpy), y_train[plan.balance], sup_train[plan.balance])
    val_set = (_host(X_train, return_numpy), y_train) if plan.val_is_train else (_host(X_val, return_numpy), y[plan.split:])
    return train_set, val_set, plan.n_classes, plan.w_classes
