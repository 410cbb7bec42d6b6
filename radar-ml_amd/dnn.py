"""Multi-view CNN classifier of the reference's ``dnn.py`` on PyTorch-ROCm: the forward pass, and its training (``Classifier.fit``,
:func:`train`: one float32 HIP step per batch, csrc/dnn_train.hip + csrc/optim.hip).

Architecture (dnn.py:45-91; shapes in images/dnn_model.png): per projection branch
Conv2D(64, 3x3, stride 2, 'same', relu) -> Conv2D(32, 3x3, stride 2, 'same', relu); concatenate the three
branches on the channel axis (order xz, yz, xy); Flatten (NHWC order, 20*20*96 = 38 400); Dense 64 relu;
Dropout 0.5; Dense 64 relu; Dropout 0.5; Dense n_classes softmax.  Keras semantics kept: TF 'same' padding
(bottom/right on even sizes), NHWC flatten order, Glorot-uniform kernels / zero biases (Keras defaults).
BASELINE config 4 runs the forward in bf16 (autocast); the dense and conv layers go to MIOpen / hipBLASLt
through PyTorch, which the north star allows for these layers.
"""
import numpy as np

from . import dnn_guard
from . import prep
from .dnn_guard import LABEL_GUARD, LABEL_GUARD_X3, LABEL_GUARD_X6, LABEL_GUARD_F32      # noqa: F401  (the margin guard's levels)
from .dnn_guard import rescore_route      # noqa: F401  (lives with the re-scoring passes both classifiers share; importable here as before)
from .nn_common import make_same_conv, to_nchw, flatten_nhwc, tf_same_pad

RESCALE = (80, 80)          # dnn.py:33
rng = np.random.default_rng(prep.RANDOM_SEED)       # dnn.py:30: the noise draws and the shuffle of preprocess_data


def _rng(given):
    return given if given is not None else rng


class History:
    """What Keras' ``model.fit`` returns: ``.history`` maps loss / accuracy / val_loss / val_accuracy to one value per epoch run."""

    def __init__(self, with_val):
        self.epoch = []
        self.history = {"loss": [], "accuracy": []}
        if with_val:
            self.history.update({"val_loss": [], "val_accuracy": []})
        self.stopped_epoch = None           # epoch index at which early stopping ended the run (None: ran all epochs)


class FitJob:
    """The data of one ``fit`` / ``train_on_batch`` call as the device function takes it.  ``xs``: three (N, H, W) float32 arrays, ``y``
    (N,) int32, ``val_xs`` / ``val_y`` the same or None, ``class_weight`` (C,) float32 (training only: Keras weighs no validation
    sample), ``batch_size``, dropout ``rate``, ``seed``; ``trusted``: the labels were checked on the host, so the status word is read
    with the epoch's results and not before every update.  ``dev``: what the device function keeps between epochs."""

    def __init__(self, xs, y, val_xs, val_y, class_weight, batch_size, rate, seed, trusted):
        self.xs, self.y, self.val_xs, self.val_y = xs, y, val_xs, val_y
        self.class_weight, self.batch_size, self.rate, self.seed, self.trusted = class_weight, int(batch_size), float(rate), int(seed), trusted
        self.dev = None          # resident tensors (_fit_upload)
        self.fit = None          # the _DeviceFit of this job


def _k2_layout(params):
    """0: the second convolution kernels are dense (out, in, ky, kx); 1: channels_last (rml_dnn_train_step's k2_layout)"""
    got = {tuple(params[4 * b + 2].stride()) for b in range(3)}
    if got == {(576, 9, 3, 1)}:
        return 0
    if got == {(576, 1, 192, 64)}:
        return 1
    raise ValueError("fit: the second convolution kernels must all be contiguous or all channels_last, got strides %s" % sorted(got))


def _fit_upload(model, job, dev):
    import torch
    from . import _lib
    lib = _lib.load()
    N, H, W = job.xs[0].shape
    C = model.n_classes
    if not lib.rml_dnn_train_supported(int(H), int(W), int(C)):
        raise _lib.RadarMLError("fit: %d x %d planes with %d classes have no training kernel (H, W multiples of 4, W <= 128, 2..16 classes)" % (H, W, C))
    if not 1 <= job.batch_size <= _lib.DNN_TRAIN_MAX_BATCH:
        raise ValueError("fit: batch_size must be in 1..%d" % _lib.DNN_TRAIN_MAX_BATCH)
    params = list(model.parameters())
    if len(params) != 18 or any(p.dtype != torch.float32 or not p.is_cuda for p in params) or model.flat_features != (H // 4) * (W // 4) * 96:
        raise ValueError("fit: the three-branch float32 model of define_classifier on a CUDA device, built for these planes, expected")
    # a contiguous CUDA float32 tensor on the model's device (what preprocess_data(return_numpy=False) returns) stays as it is
    up = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()        # noqa: E731
    st = {"x": [up(a, torch.float32) for a in job.xs], "y": up(job.y, torch.int32), "N": int(N), "H": int(H), "W": int(W),
          "cw": up(job.class_weight, torch.float32), "acc": torch.zeros((4,), dtype=torch.float64, device=dev)}
    if job.val_xs is not None:
        st["vx"] = [up(a, torch.float32) for a in job.val_xs]
        st["vy"] = up(job.val_y, torch.int32)
        st["vrows"] = torch.arange(len(job.val_y), dtype=torch.int32, device=dev)
    # one workspace for every call of the fit: rml_dnn_train_workspace_bytes(B) covers every batch of up to B samples -- the partial
    # last batch of an epoch included -- and validation runs in batches of up to DNN_TRAIN_MAX_BATCH whatever batch_size is
    top = max(job.batch_size, min(_lib.DNN_TRAIN_MAX_BATCH, len(job.val_y)) if job.val_xs is not None else 0)
    nbytes = int(lib.rml_dnn_train_workspace_bytes(int(top), int(H), int(W), int(C)))
    st["ws"], st["ws_bytes"] = torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes
    job.dev = st
    return st


class _DeviceFit:
    """The enqueueing half of :func:`_fit_epoch` for one (model, job): ``train`` queues one update (rml_dnn_train_step +
    rml_adam_step) on a batch of resident rows, ``validate`` the eval-mode pass over the validation set; neither reads device memory.
    ``acc``: loss sum | val loss sum (float64) | correct, val correct | status, pad (int32)."""

    def __init__(self, model, job):
        import ctypes as C
        import torch
        from . import _lib
        from .nn_common import DeviceAdam
        self.C, self.torch, self._lib, self.lib = C, torch, _lib, _lib.load()
        self.model, self.job = model, job
        self.params = params = list(model.parameters())
        self.dev = dev = params[0].device
        if dev.type != "cuda":
            raise _lib.RadarMLError("fit runs on the GPU: move the model to a CUDA device (there is no CPU path)")
        self.st = job.dev if job.dev is not None else _fit_upload(model, job, dev)
        opt = model._opt
        if model._adam is None or model._adam.params[0] is not params[0]:
            model._adam = DeviceAdam(params, opt["lr"], (opt["beta_1"], opt["beta_2"]), opt["epsilon"])
            model._grads = [torch.empty_like(p) for p in params]
        self.adam, self.grads = model._adam, model._grads
        self.pp = (C.c_void_p * 18)(*[p.data_ptr() for p in params])
        self.gp = (C.c_void_p * 18)(*[g.data_ptr() for g in self.grads])
        self.layout = _k2_layout(params)
        self.acc = self.st["acc"]
        self.ctx = _lib.context(dev)

    def _step(self, x, y, N, rows, off, B, cw, mode, t, slot):
        C, _lib, st, a0 = self.C, self._lib, self.st, self.acc.data_ptr()
        _lib.check(self.lib.rml_dnn_train_step(self.ctx, _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(x[2]), _lib.ptr(y), C.c_void_p(rows.data_ptr() + 4 * off),
                                               B, N, st["H"], st["W"], _lib.ptr(cw), self.model.n_classes, self.pp, self.gp, self.layout, self.job.seed,
                                               t, self.job.rate, mode, _lib.ptr(st["ws"]), st["ws_bytes"], C.c_void_p(a0 + 8 * slot),
                                               C.c_void_p(a0 + 16 + 4 * slot), C.c_void_p(a0 + 24), _lib.stream_ptr(self.dev)), "rml_dnn_train_step")

    def status(self):
        """the status word, read now (a device synchronisation)"""
        return int(self.acc.view(self.torch.int32)[6].item())

    def train(self, rows, off, B, check_status=False):
        """one update on rows[off : off + B] (``rows``: int32 device tensor of indices into the resident training set)"""
        st, model = self.st, self.model
        self._step(st["x"], st["y"], st["N"], rows, off, B, st["cw"], self._lib.DNN_TRAIN, model._train_steps, 0)
        # A set status means the step wrote no gradient: the update must not run on the previous batch's.  Callers that cannot rule
        # it out on the host (train_on_batch) look before the update; fit has checked every label and makes the row indices itself.
        if check_status and self.status() != 0:
            self.bad_status()
        self.adam.step(self.grads)
        model._train_steps += 1

    def validate(self):
        st, top = self.st, self._lib.DNN_TRAIN_MAX_BATCH
        nv = int(st["vy"].numel())
        for off in range(0, nv, top):
            self._step(st["vx"], st["vy"], nv, st["vrows"], off, min(top, nv - off), None, self._lib.DNN_EVAL, 0, 1)

    def bad_status(self):
        raise self._lib.RadarMLError("rml_dnn_train_step: a row index outside [0, N) or a label outside [0, n_classes) (status -1): no update was made")


def _fit_epoch(model, job, perm):
    """ALL device work of ``fit`` / ``train_on_batch``: one epoch over the training rows in the order ``perm`` (int32) in batches of
    ``job.batch_size`` -- rml_dnn_train_step + rml_adam_step per batch, on resident data (uploaded at the first call) -- then the
    validation set in eval mode.  Returns (loss sum, correct, val loss sum, val correct) from ONE read of device memory.  The module's
    parameters are trained in place.  Tests replace this function by a float64 CPU restatement (tests/dnn_train_common.py)."""
    import torch
    f = job.fit if job.fit is not None and job.fit.params[0] is next(model.parameters()) else _DeviceFit(model, job)
    job.fit = f
    assert job.trusted or len(perm) <= job.batch_size       # an unchecked job is one batch, whose status is read before its update
    with torch.no_grad(), torch.cuda.device(f.dev):
        f.acc.zero_()
        rows = torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).to(f.dev)
        for off in range(0, len(perm), job.batch_size):
            f.train(rows, off, min(job.batch_size, len(perm) - off), check_status=not job.trusted)
        if "vx" in f.st:
            f.validate()
        host = f.acc.cpu()
    # the library wrote the parameters through raw pointers: tell torch (the weight packs of _cached key on the version counters)
    for p in f.params:
        torch.autograd.graph.increment_version(p)
    ints = host.view(torch.int32)
    if int(ints[6]) != 0:
        f.bad_status()
    return float(host[0]), int(ints[4]), float(host[1]), int(ints[5])


def _planes(a):
    """(N, H, W) float32 from what Keras feeds: (N, H, W) or (N, H, W, 1) arrays (or tensors).  NumPy for host data; a CUDA tensor stays
    on its device (contiguous float32 ones as they are), so a data set prepared there is not pulled back to be uploaded again."""
    on_dev = hasattr(a, "detach") and a.is_cuda
    a = a.detach() if on_dev else (a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a))
    if a.ndim == 4 and a.shape[-1] == 1:
        a = a[..., 0]
    if a.ndim != 3:
        raise ValueError("expected (N,H,W) or (N,H,W,1), got %s" % (tuple(a.shape),))
    if on_dev:
        import torch
        return a.to(torch.float32).contiguous()
    return np.ascontiguousarray(a, dtype=np.float32)


def _labels(y):
    """(N,) host array of the labels (a tensor is read back: N integers)"""
    return (y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)).reshape(-1)


def _class_weights(class_weight, n_classes):
    """Keras' ``class_weight`` dict {class index: weight} (classes it leaves out weigh 1), or an array of n_classes weights"""
    w = np.ones((n_classes,), np.float32)
    if class_weight is None:
        return w
    if isinstance(class_weight, dict):
        for k, v in class_weight.items():
            if not 0 <= int(k) < n_classes:
                raise ValueError("class_weight: class %r of %d" % (k, n_classes))
            w[int(k)] = v
        return w
    w = np.asarray(class_weight, dtype=np.float32).reshape(-1)
    if len(w) != n_classes:
        raise ValueError("class_weight: %d weights for %d classes" % (len(w), n_classes))
    return w


def augment_data(x, rotation_range=1.0, zoom_range=0.3, noise_sd=1.0, rng=None, device=None):
    """``augment_data`` of dnn.py:94-182 on the GPU (one ``rml_augment_chain`` launch per projection): ``x`` = (xz, yz, xy) already in
    [-1, 1]; rotate every projection by its own angle, zoom all by one factor, add one noise draw per projection, clamp to [-1, 1] after
    each stage.  Same arguments and order of draws as the reference: one ``np.random.uniform`` per projection for the angles, one for
    the zoom factor, one ``rng.normal(scale=noise_sd)`` per projection from this module's ``rng`` (``default_rng(1234)``) unless ``rng``
    is given; a range that is None skips its stage and its draws.  Returns float32 planes (integer / float64 input is converted first):
    NumPy arrays, or CUDA tensors where ``x`` held CUDA tensors."""
    return prep.augment_data(x, rotation_range, zoom_range, noise_sd, _rng(rng), device)


def preprocess_data(args, data, labels, *, rng=None, device=None, return_numpy=True):
    """``preprocess_data`` of dnn.py:185-277 with the arrays on the GPU.  ``args``: anything with ``.augment`` and ``.train_split``;
    ``data``: [(xz, yz, xy), ...] planes in [0, 255] (arenas may be mixed); ``labels``: one name per sample.  Returns
    ``X_train, y_train, X_val, y_val, n_classes, w_classes`` as the reference does: (N, 80, 80, 3) float32 in [-1, 1], label-encoded
    ``y``, ``w_classes = {cls: round(largest class / n, 2)}``.

    All draws of the data set are made first, on the host, in the reference's order (see :func:`augment_data`); ``rng.shuffle`` of the
    index follows the noise draws on the same generator (this module's ``rng`` unless one is given), so a seeded run gives the
    reference's data set in the reference's order.  Then one ``rml_augment_chain`` and one ``rml_resize_bicubic`` launch per (projection,
    plane shape); shuffle and split are one device gather.  Without ``augment`` the result is bit-identical to the reference's; with it
    the spline stages are within 4e-6 each.  ``return_numpy=False`` leaves ``X_train`` / ``X_val`` as CUDA tensors,
    which ``fit`` / ``train`` take without a host round trip.  Planes are handled in float32: integer / float64 data-set planes are
    converted first (the reference would scale those in float64)."""
    return prep.preprocess_dnn(args, data, labels, RESCALE, _rng(rng), device, return_numpy)


def train(model, X, y, X_val, y_val, w_classes, results_dir, epochs=100, patience=10, logger=None):
    """dnn.py:347-390: fit with batches of 64, up to 100 epochs, class weights, EarlyStopping(patience=10) and
    ModelCheckpoint(save_best_only) on val_loss -- the best weights go to ``results_dir/c_model.pt`` (a ``state_dict``) -- and
    the reference's log lines.  ``X``, ``X_val``: (N, H, W, 3) arrays or CUDA tensors (``preprocess_data(return_numpy=False)``), the
    projections xz, yz, xy on the last axis.  Returns the history."""
    import logging
    import os
    log = logger or logging.getLogger(__name__)
    fp = os.path.join(results_dir, "c_model.pt")
    log.info("Training model.")
    hist = model.fit(x=[X[..., 0], X[..., 1], X[..., 2]], y=y, batch_size=64, epochs=epochs,
                     validation_data=([X_val[..., 0], X_val[..., 1], X_val[..., 2]], y_val), class_weight=w_classes, patience=patience,
                     checkpoint=fp)
    if hist.stopped_epoch is not None:
        log.info("Epoch %d: early stopping" % (hist.stopped_epoch + 1))
    best_val_loss = min(hist.history["val_loss"])
    i = hist.history["val_loss"].index(best_val_loss)
    log.info("Best loss: %.4f, Best acc: %.2f%%" % (hist.history["loss"][i], hist.history["accuracy"][i] * 100))
    log.info("Best val loss: %.4f, Best val acc: %.2f%%" % (best_val_loss, hist.history["val_accuracy"][i] * 100))
    log.info("Saved best model to %s" % results_dir)
    return hist


def define_classifier(xz_shape=(80, 80, 1), yz_shape=(80, 80, 1), xy_shape=(80, 80, 1), n_classes=3,
                      device=None, dtype=None):
    """Same signature/ordering as dnn.define_classifier (dnn.py:55): input order xz, yz, xy.
    Returns a ``Classifier`` with Keras-like ``predict``."""
    import torch
    m = Classifier([xz_shape, yz_shape, xy_shape], n_classes)
    dev = torch.device(device) if device is not None else (
        torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    return m.to(dev).to(memory_format=torch.channels_last)


def _module_base():
    import torch.nn as nn
    return nn.Module


class Classifier(dnn_guard.ExactRescore, _module_base()):
    def __init__(self, shapes, n_classes):
        import torch
        import torch.nn as nn
        super().__init__()
        self.shapes = [tuple(s) for s in shapes]
        self.n_classes = n_classes
        self.branches = nn.ModuleList()
        feat = 0
        for (h, w, c) in self.shapes:
            self.branches.append(nn.ModuleList([make_same_conv(c, 64, 3, 2), make_same_conv(64, 32, 3, 2)]))
            feat += (-(-(-(-h // 2)) // 2)) * (-(-(-(-w // 2)) // 2)) * 32
        self.flat_features = feat
        self.fc1 = nn.Linear(feat, 64)
        self.fc2 = nn.Linear(64, 64)
        self.fc3 = nn.Linear(64, n_classes)
        self.drop = nn.Dropout(0.5)
        self._packs = {}                            # name -> (key of the parameters it was made from, value): _cached
        self._margin = dnn_guard.MarginGuard()
        self._opt, self._adam, self._grads, self._train_steps, self._rng = None, None, None, 0, None     # training: compile()
        # Keras defaults: glorot_uniform kernels, zero biases
        for mod in self.modules():
            if isinstance(mod, (nn.Conv2d, nn.Linear)):
                nn.init.xavier_uniform_(mod.weight)
                nn.init.zeros_(mod.bias)

    def features(self, xz, yz, xy):
        import torch
        import torch.nn.functional as F
        outs = []
        for x, br in zip((xz, yz, xy), self.branches):
            x = F.relu(br[0](x))
            x = F.relu(br[1](x))
            outs.append(x)
        # all three branches share the spatial size after RESCALE; concat on channels like Keras' last axis
        return flatten_nhwc(torch.cat(outs, dim=1))

    def logits(self, xz, yz, xy):
        import torch.nn.functional as F
        fv = self.features(xz, yz, xy)
        h = self.drop(F.relu(self.fc1(fv)))
        h = self.drop(F.relu(self.fc2(h)))
        return self.fc3(h)

    def forward(self, xz, yz, xy):
        import torch
        return torch.softmax(self.logits(xz, yz, xy).float(), dim=-1)

    def keras_weights(self):
        """The parameters in Keras layout (conv kernels (kh,kw,cin,cout), dense kernels (in,out)) as float64 numpy:
        (conv_weights per branch [(k1,b1,k2,b2)], dense_weights [(kernel,bias)]*3) -- what ``model.get_weights()``
        of the reference's Keras model holds, and what the oracle's restatement takes."""
        def k(conv):
            return conv.weight.detach().double().permute(2, 3, 1, 0).cpu().numpy(), conv.bias.detach().double().cpu().numpy()
        convs = []
        for br in self.branches:
            k1, b1 = k(br[0].conv)
            k2, b2 = k(br[1].conv)
            convs.append((k1, b1, k2, b2))
        dense = [(fc.weight.detach().double().t().cpu().numpy(), fc.bias.detach().double().cpu().numpy())
                 for fc in (self.fc1, self.fc2, self.fc3)]
        return convs, dense

    def set_keras_weights(self, convs, dense):
        """Inverse of :meth:`keras_weights`: load parameters that come in Keras layout -- conv kernels (kh, kw, cin, cout),
        dense kernels (in, out), the three branches in input order xz, yz, xy -- i.e. the arrays a maintainer gets from the
        reference's trained model (``tf.keras.models.load_model(...)``, dnn.py:364-370, then ``layer.get_weights()`` per
        layer).  The flatten order needs no permutation: features() already flattens NHWC like Keras."""
        import torch
        if len(convs) != len(self.branches) or len(dense) != 3:
            raise ValueError("expected %d conv branches of (k1, b1, k2, b2) and 3 dense (kernel, bias) pairs" % len(self.branches))

        def put(param, arr, what):
            t = torch.as_tensor(np.asarray(arr), dtype=param.dtype)
            if tuple(t.shape) != tuple(param.shape):
                raise ValueError("%s: Keras array gives %s, the layer holds %s" % (what, tuple(t.shape), tuple(param.shape)))
            param.copy_(t.to(param.device))

        with torch.no_grad():
            for bi, (br, (k1, b1, k2, b2)) in enumerate(zip(self.branches, convs)):
                for conv, k, b, nm in ((br[0].conv, k1, b1, "conv1"), (br[1].conv, k2, b2, "conv2")):
                    k = np.asarray(k)
                    if k.ndim != 4:
                        raise ValueError("branch %d %s kernel: expected (kh, kw, cin, cout)" % (bi, nm))
                    put(conv.weight, k.transpose(3, 2, 0, 1), "branch %d %s kernel" % (bi, nm))
                    put(conv.bias, b, "branch %d %s bias" % (bi, nm))
            for fc, (k, b), nm in zip((self.fc1, self.fc2, self.fc3), dense, ("dense", "dense_1", "dense_2")):
                put(fc.weight, np.asarray(k).T, nm + " kernel")
                put(fc.bias, b, nm + " bias")
        return self

    def set_keras_weight_list(self, weights, order="depth"):
        """Load the flat list ``model.get_weights()`` returns for the reference's functional model (dnn.py:55-91).
        Keras lists a functional model's layers by graph depth, so the three first convolutions (xz, yz, xy) come before
        the three second ones: ``order="depth"``; ``order="branch"`` takes [xz conv1, xz conv2, yz conv1, ...] instead.
        (No TensorFlow here to confirm the order on a live model -- the shapes are checked, the order is the caller's.)"""
        w = [np.asarray(a) for a in weights]
        nb = len(self.branches)
        if len(w) != 4 * nb + 6:
            raise ValueError("expected %d arrays (kernel + bias of %d convolutions and 3 dense layers), got %d" % (4 * nb + 6, 2 * nb, len(w)))
        if order == "depth":
            convs = [(w[2 * b], w[2 * b + 1], w[2 * nb + 2 * b], w[2 * nb + 2 * b + 1]) for b in range(nb)]
        elif order == "branch":
            convs = [tuple(w[4 * b:4 * b + 4]) for b in range(nb)]
        else:
            raise ValueError("order must be 'depth' or 'branch'")
        d = w[4 * nb:]
        return self.set_keras_weights(convs, [(d[0], d[1]), (d[2], d[3]), (d[4], d[5])])

    def evaluate(self, inputs, y, batch_size=8192, autocast_dtype=None):
        """Keras ``model.evaluate([xz, yz, xy], y)`` of the compiled classifier (dnn.py:88-90: sparse categorical
        cross-entropy + accuracy): returns (loss, accuracy), the means over all samples, dropout inactive."""
        p = self.predict(inputs, batch_size=batch_size, autocast_dtype=autocast_dtype).astype(np.float64)
        yi = np.asarray(y).reshape(-1).astype(np.int64)
        if len(yi) != len(p):
            raise ValueError("evaluate: %d label(s) for %d sample(s)" % (len(yi), len(p)))
        if len(yi) == 0:
            return 0.0, 0.0
        # Keras clips the probabilities to [1e-7, 1 - 1e-7] before the log (backend.sparse_categorical_crossentropy)
        pt = np.clip(p[np.arange(len(yi)), yi], 1e-7, 1.0 - 1e-7)
        return float(-np.log(pt).mean()), float((p.argmax(axis=1) == yi).mean())

    # ---- weight packs: values derived from parameters, rebuilt when one of them was written ------------------
    def _cached(self, name, params, make):
        """``make()``, kept under ``name`` until one of ``params`` is written (optimizer step, load_state_dict, .to(): the tensors'
        version counters / storage change -- dnn_guard.weights_key)."""
        key = dnn_guard.weights_key(params)
        hit = self._packs.get(name)
        if hit is None or hit[0] != key:
            hit = self._packs[name] = (key, make())
        return hit[1]

    def _conv_packs(self):
        """The convolution weights in the layout of the trunk kernels: w1 [3][64][9], b1 [3][64], w2 [3][32][576] with k = (ky*3+kx)*64
        + cin, b2 [3][32], float32 -- ``["x3"]`` for rml_dnn_trunk_x3 as they are, ``["bf16"]`` for rml_dnn_trunk with w2 in bf16."""
        import torch

        def make():
            w1 = torch.stack([br[0].conv.weight.detach().float().reshape(64, 9) for br in self.branches]).contiguous()
            b1 = torch.stack([br[0].conv.bias.detach().float() for br in self.branches]).contiguous()
            # (32, 64, 3, 3) -> (32, ky, kx, cin) -> (32, 576)
            w2 = torch.stack([br[1].conv.weight.detach().float().permute(0, 2, 3, 1).reshape(32, 576) for br in self.branches]).contiguous()
            b2 = torch.stack([br[1].conv.bias.detach().float() for br in self.branches]).contiguous()
            return {"x3": (w1, b1, w2, b2), "bf16": (w1, b1, w2.to(torch.bfloat16).contiguous(), b2)}
        return self._cached("conv", [p for br in self.branches for cv in (br[0].conv, br[1].conv) for p in (cv.weight, cv.bias)], make)

    def _dense_packs(self):
        """The dense kernels in the layouts the tails use.  ``["bf16"]``: (kernel, bias) copies per layer for the matrix cores (autocast
        re-casts the three weight matrices on every call: six element-wise launches of ~6 us per batch in the round-3 profile);
        ``["f32"]``: the float32 operands of csrc/dense.hip's small layers (b1, second kernel transposed to (in, out), b2, w3, b3);
        ``["w1_kblock"]``: the first bf16 kernel with its K axis in the K-block order (branch, pixel, channel) instead of Keras'
        (pixel, branch, channel), blocked like the features: [K/64][out][64] (None unless K % 192 == 0)."""
        import torch
        fcs = (self.fc1, self.fc2, self.fc3)

        def make():
            bf16 = [(fc.weight.detach().to(torch.bfloat16).contiguous(), fc.bias.detach().to(torch.bfloat16).contiguous()) for fc in fcs]
            f32 = (self.fc1.bias.detach().float().contiguous(), self.fc2.weight.detach().float().t().contiguous(),
                   self.fc2.bias.detach().float().contiguous(), self.fc3.weight.detach().float().contiguous(),
                   self.fc3.bias.detach().float().contiguous())
            w1 = bf16[0][0]
            K = int(w1.shape[1])
            kblock = (w1.view(w1.shape[0], K // 96, 3, 32).permute(0, 2, 1, 3).reshape(w1.shape[0], K // 64, 64)
                      .permute(1, 0, 2).contiguous() if K % 192 == 0 else None)
            return {"bf16": bf16, "f32": f32, "w1_kblock": kblock}
        return self._cached("dense", [p for fc in fcs for p in (fc.weight, fc.bias)], make)

    def _tail_weights(self):
        return self._dense_packs()["bf16"]

    @property
    def _tail_f32(self):
        return self._dense_packs()["f32"]

    def _exact_weights(self, dtype):
        """float32 / float64 copies of every parameter in the layout of forward_exact, cached until one is written."""
        made = self._cached("exact", self.parameters(), dict)
        if dtype not in made:
            made[dtype] = {
                "conv": [[(cv.conv.weight.detach().to(dtype).reshape(cv.conv.weight.shape[0], -1).contiguous(), cv.conv.bias.detach().to(dtype),
                           int(cv.conv.weight.shape[2]), int(cv.conv.weight.shape[3])) for cv in br] for br in self.branches],
                "fc": [(fc.weight.detach().to(dtype), fc.bias.detach().to(dtype)) for fc in (self.fc1, self.fc2, self.fc3)]}
        return made[dtype]

    # ---- fused HIP trunk + dense tail: the bf16 chain ----------------------------------------------------
    def features_fused(self, xz, yz, xy, layout="nhwc"):
        """The conv features (bf16) of the three branches from the fused HIP kernel (csrc/dnn.hip); inputs (N,H,W) or
        (N,1,H,W) CUDA tensors, float32 or bfloat16 (same results).  ``layout="nhwc"``: (N, 38 400) rows in Keras' Flatten
        order; ``layout="kblock"``: the same values as (K/64, N, 64) with the K axis ordered (branch, pixel, channel) -- what
        ``dense_tail(..., kblock=True)`` streams (rml_dnn_trunk_kblock)."""
        import torch
        from . import _lib
        lib = _lib.load()
        bf = all(x.dtype == torch.bfloat16 for x in (xz, yz, xy))
        xs = [x.reshape(x.shape[0], x.shape[-2], x.shape[-1]) for x in (xz, yz, xy)]
        xs = [(x if bf else x.float()).contiguous() for x in xs]
        n, H, W = xs[0].shape
        dev = xs[0].device
        w1, b1, w2t, b2 = self._conv_packs()["bf16"]
        K = (H // 4) * (W // 4) * 96
        kb = layout == "kblock"
        if not kb and layout != "nhwc":
            raise ValueError("layout must be 'nhwc' or 'kblock'")
        feat = torch.empty((K // 64, n, 64) if kb else (n, K), dtype=torch.bfloat16, device=dev)
        fn = lib.rml_dnn_trunk_kblock if kb else lib.rml_dnn_trunk
        with torch.cuda.device(dev):
            _lib.check(fn(_lib.context(dev), _lib.ptr(xs[0]), _lib.ptr(xs[1]), _lib.ptr(xs[2]), 1 if bf else 0,
                          n, H, W, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2t), _lib.ptr(b2), _lib.ptr(feat),
                          _lib.stream_ptr(dev)), "rml_dnn_trunk")
        return feat

    def _small_tail_shape(self):
        """the reference's 64 / 64 / n dense layers, as csrc/dense.hip's finishing kernels take them"""
        return tuple(self.fc2.weight.shape) == (64, 64) and self.fc1.weight.shape[0] == 64 and self.n_classes <= 16

    def kblock_supported(self, H, W):
        """True when trunk and dense tail can hand the features over in the K-block layout: planes the register-resident trunk
        kernel takes (rml_dnn_trunk_kblock_supported answers from the kernel's own LDS layout; the 80 x 80 of dnn.py does), the
        reference's three branches and 64 / 64 / n dense layers on those planes."""
        from . import _lib
        return (len(self.branches) == 3 and self._small_tail_shape() and self.fc1.weight.shape[1] == (H // 4) * (W // 4) * 96
                and bool(_lib.load().rml_dnn_trunk_kblock_supported(int(H), int(W))))

    def forward_fused(self, xz, yz, xy):
        """Class probabilities with the fused HIP trunk + the fused dense tail (csrc/dense.hip)."""
        H, W = int(xz.shape[-2]), int(xz.shape[-1])
        if self.kblock_supported(H, W):
            return self.dense_tail(self.features_fused(xz, yz, xy, layout="kblock"), kblock=True)
        return self.dense_tail(self.features_fused(xz, yz, xy))

    def _hip_tail(self, name, fv, lead, n, K, w1, small, ws_bytes):
        """csrc/dense.hip's tail ``name`` (rml_dnn_dense_tail / _f32) on the features ``fv``: ``lead`` are its arguments between
        the features and n, ``w1`` the first kernel as it takes it, ``small`` = _dense_packs()["f32"], ``ws_bytes(ctx)`` its
        workspace size."""
        import torch
        from . import _lib
        dev = fv.device
        out = torch.empty((n, self.n_classes), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        bb1, w2t, bb2, w3f, bb3 = small
        ctx = _lib.context(dev)
        nbytes = int(ws_bytes(ctx))
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(getattr(_lib.load(), name)(ctx, _lib.ptr(fv), *lead, n, K, _lib.ptr(w1), _lib.ptr(bb1), _lib.ptr(w2t), _lib.ptr(bb2),
                                                  _lib.ptr(w3f), _lib.ptr(bb3), self.n_classes, _lib.ptr(ws), nbytes, _lib.ptr(out),
                                                  _lib.stream_ptr(dev)), name)
        return out

    @staticmethod
    def _torch_tail(fv, layers):
        """Dense relu, Dense relu, Dense softmax through PyTorch (hipBLASLt), float32 accumulation and softmax: the tails' form for
        the shapes and devices csrc/dense.hip does not take."""
        import torch
        import torch.nn.functional as F
        (w1, b1), (w2, b2), (w3, b3) = layers
        h = F.relu(F.linear(fv, w1, b1))
        h = F.relu(F.linear(h, w2, b2))
        return torch.softmax(F.linear(h, w3, b3).float(), dim=-1)

    def dense_tail(self, fv, fused=True, kblock=False):
        """Dense 64 relu, Dense 64 relu, Dense n softmax (dnn.py:78-88) on bf16 feature rows.  ``fused`` (default, CUDA bf16 rows
        with K % 64 == 0, two hidden layers of 64 units, <= 16 classes): csrc/dense.hip -- the first layer as a split-K bf16 GEMM
        that streams the rows once, the small layers and the softmax in float32 in one finishing kernel.  Otherwise the
        arithmetic of the autocast region (hipBLASLt through PyTorch: bf16 operands, float32 accumulation, bf16 activations)
        without its per-call casts.  ``kblock=True``: ``fv`` is the (K/64, N, 64) tensor of ``features_fused(layout="kblock")`` --
        a 128-sample tile of a K-step is then 16 KB of contiguous memory instead of 128 pieces 76.8 KB apart."""
        import torch
        from . import _lib
        pk = self._dense_packs()
        w1 = pk["bf16"][0][0]
        if kblock:
            w1 = pk["w1_kblock"]
            if not (fused and fv.is_cuda and fv.dtype == torch.bfloat16 and fv.ndim == 3 and fv.shape[2] == 64 and fv.is_contiguous()
                    and w1 is not None and int(fv.shape[0]) == int(w1.shape[0])):
                raise ValueError("dense_tail(kblock=True): contiguous CUDA bfloat16 (K/64, N, 64) features expected")
            K, n, ld = int(fv.shape[0]) * 64, int(fv.shape[1]), 0
        else:
            K, n, ld = (int(fv.shape[1]), int(fv.shape[0]), int(fv.stride(0))) if fv.ndim == 2 else (0, 0, 0)
        if kblock or (fused and fv.is_cuda and fv.dtype == torch.bfloat16 and fv.ndim == 2 and K % 64 == 0 and fv.stride(1) == 1
                      and fv.stride(0) % 8 == 0 and fv.data_ptr() % 16 == 0 and self._small_tail_shape()):
            return self._hip_tail("rml_dnn_dense_tail", fv, (ld, 1 if kblock else 0), n, K, w1, pk["f32"],
                                  lambda ctx: _lib.load().rml_dnn_dense_workspace_bytes(ctx, n, K))
        return self._torch_tail(fv, pk["bf16"])

    def _tail_float32(self, fv):
        """Dense 64 relu, Dense 64 relu, Dense n softmax in float32 on float32 feature rows (no dropout: inference).  CUDA rows
        (two hidden layers of 64 units, <= 16 classes, K % 4 == 0): csrc/dense.hip rml_dnn_dense_tail_f32 -- a row's result depends
        on that row alone (fixed K splits, one fma chain each, added in order), so a row re-scored alone, inside any candidate set
        or twice has the same bits; hipBLASLt's float32 GEMM for these shapes splits K with atomics and does not (session r6b:
        the same call twice 1e-7 apart).  Other shapes / CPU tensors: the plain PyTorch layers."""
        import torch
        from . import _lib
        layers = self._exact_weights(torch.float32)["fc"]
        w1, w2 = layers[0][0], layers[1][0]
        if (fv.is_cuda and fv.dtype == torch.float32 and fv.ndim == 2 and fv.stride(1) == 1 and fv.shape[1] % 4 == 0 and fv.stride(0) % 4 == 0
                and fv.data_ptr() % 16 == 0 and tuple(w1.shape) == (64, int(fv.shape[1])) and tuple(w2.shape) == (64, 64) and self.n_classes <= 16):
            n, K = int(fv.shape[0]), int(fv.shape[1])
            return self._hip_tail("rml_dnn_dense_tail_f32", fv, (int(fv.stride(0)),), n, K, w1 if w1.is_contiguous() else w1.contiguous(),
                                  self._tail_f32, lambda ctx: _lib.load().rml_dnn_dense_tail_f32_workspace_bytes(n, K))
        return self._torch_tail(fv, layers)

    def _features_timed(self, xs, trunk_events, layout="nhwc"):
        import torch
        if trunk_events is None:
            return self.features_fused(*xs, layout=layout)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fv = self.features_fused(*xs, layout=layout)
        e1.record()
        trunk_events.append((e0, e1, int(xs[0].shape[0])))
        return fv

    def _forward_timed(self, xs, trunk_events):
        kb = self.kblock_supported(int(xs[0].shape[-2]), int(xs[0].shape[-1]))
        return self.dense_tail(self._features_timed(xs, trunk_events, "kblock" if kb else "nhwc"), kblock=kb)

    # ---- volumes -> probabilities --------------------------------------------------------------------------
    def predict_volumes(self, volumes, rescale=(80, 80), mode="max", batch_size=16384, overlap=False, trunk_events=None,
                        exact_resize=False, label_guard=LABEL_GUARD, ijk=None, num_targets=1, return_ijk=False):
        """The whole inference path of BASELINE configs[3] on the GPU: (N,X,Y,Z) volumes (float32 or uint8) ->
        projections as uint8 code rows (csrc/project*.hip) -> [-1,1] scaling + bicubic resize of the three projections in one
        launch, bf16 out (csrc/preprocess.hip: Pillow's windows and weights in float32) -> fused conv trunk (csrc/dnn.hip) ->
        dense tail: class probabilities (N, n_classes) as a float32 CUDA tensor.  ``exact_resize=True`` (and shapes the fused
        preprocessing does not take) runs the round-1..3 chain instead: float32 feature rows and the Pillow-bit-identical
        float64 resize (csrc/resize.hip), one launch per projection -- the same values before the bf16 rounding to ~1e-6.

        ``batch_size``: frames per pass of the chain (16 384: 5.96-6.08 M frames/s against 5.83-5.85 M at 8 192 and 6.03-6.04 M at
        32 768 on one box -- fewer launch gaps and persistent-kernel tails; 2.2 GB of intermediates at the Walabot grid).
        ``overlap`` (off): the two-stream chain (:meth:`_chain_two_streams`; measured: no gain, kept as a knob).  ``trunk_events``:
        a list that receives one (start, stop, frames) torch.cuda.Event triple per trunk launch (bench.py's in-situ roofline of
        k_dnn_trunk_rf).

        ``label_guard`` (default LABEL_GUARD = 2e-2; None or 0 turns it off): the margin guard (:meth:`_guard`, dnn_guard.py).  The bf16
        chain moves a probability by up to 3.4e-3 (measured against the float64 restatement of the Keras layers, trained weights;
        4.8e-4 on random-init ones), so rows whose two largest probabilities are closer than ``label_guard`` -- and only those -- are
        scored again from their volumes from exact inputs (exact projection, Pillow-bit-identical resize: :meth:`rescore_exact`) and
        replaced; the gap widens itself to four times the bf16 error seen on them -- an EMPIRICAL bound: ``argmax`` is the float64
        label on every row inside the covered gap and on every row outside it whose bf16 error is below twice the largest error
        seen.  Guarded outputs are not batching-invariant bit for bit (a row near the gap may be re-scored under one batching and
        not under another; both values are within the bf16 tolerance); ``label_guard=None`` results are.  ``self.last_guard``: what
        the guard did (the keys: dnn_guard.py).

        ``mode="slice"``: what the model was trained on -- the three planes of the image through a target's voxel, yz = V[i,:,:],
        xz = V[:,j,:], xy = V[:,:,k] (predict.py:98-107), for every target of every frame (predict.py:93-119).  ``ijk``: (N,3) or
        (N,T,3) indices (negative ones wrap like Python's); None: the ``num_targets`` strongest derived targets of every frame
        (``common.derive_targets``).  The result has N*T rows, frame-major (row b*T+t is target t of frame b); ``return_ijk=True``
        returns ``(proba, ijk)`` with the (N,T,3) int32 indices the rows were sliced at.  (N,T,3) and derived targets go from the
        volumes into the preprocessing kernel's LDS image in one launch (csrc/preprocess_slice.hip); the margin guard re-scores
        row r from frame r // T at ijk[r] (:meth:`rescore_exact`).  The other modes ignore the three arguments.
        """
        import torch
        if not isinstance(volumes, torch.Tensor):
            volumes = torch.as_tensor(volumes)
        n = int(volumes.shape[0])
        dev = volumes.device if volumes.is_cuda else next(self.parameters()).device
        sliced = mode == "slice"
        T = 1
        if sliced:
            from . import nn_common
            ijk, T = nn_common.slice_targets_arg(ijk, n, num_targets)
        if n == 0:
            res = torch.zeros((0, self.n_classes), device=dev)
            return (res, torch.zeros((0, T, 3), dtype=torch.int32, device=dev)) if (sliced and return_ijk) else res
        if dev.type != "cuda":
            raise RuntimeError("predict_volumes runs on the GPU: move the model to a CUDA device (there is no CPU path)")
        bs = int(min(batch_size, n))
        plan = [(s0, min(n, s0 + bs)) for s0 in range(0, n, bs)]         # the passes: frames [s0, s1) each
        out = torch.empty((n * T, self.n_classes), dtype=torch.float32, device=dev)
        if sliced:
            with torch.no_grad(), torch.cuda.device(dev):
                used = self._chain_slices(volumes, plan, out, rescale, exact_resize, trunk_events, ijk, T)
                res = self._guard(out, label_guard, lambda idx, prec: self.rescore_exact(volumes, rescale, mode, prec, rows=idx, ijk=used))
            return (res, used) if return_ijk else res
        with torch.no_grad(), torch.cuda.device(dev):
            if overlap and len(plan) > 1 and volumes.is_cuda:
                self._chain_two_streams(volumes, plan, out, rescale, mode, trunk_events)
            else:
                self._chain_serial(volumes, plan, out, rescale, mode, exact_resize, trunk_events)
            # the margin guard once per call, behind the last pass.  (Per pass on a second stream beside the next pass, with a
            # context of its own, was measured in session r5f: no overlap -- the chain's persistent kernels hold every CU and
            # the guard's small launches start only at kernel boundaries -- and more padded chunks: 58 % against ~35 %.)
            return self._guard(out, label_guard, lambda idx, prec: self.rescore_exact(volumes, rescale, mode, prec, rows=idx))

    def _chain_serial(self, volumes, plan, out, rescale, mode, exact_resize, trunk_events):
        """One pass after the other on the caller's stream.  Host volumes stay on the host: one slice per pass crosses PCIe, not the
        whole data set."""
        from . import common, nn_common
        dims = tuple(int(v) for v in volumes.shape[1:])
        dev = out.device
        # (mode "max_nan" can put NaN into the float rows: the fused float32 preprocessing multiplies out-of-window taps by
        # zero weights, 0 * NaN, where Pillow never reads them -- those batches take the Pillow-exact resize)
        fused = not exact_resize and mode != "max_nan" and nn_common.preprocess_supported(dims, rescale)
        for s0, s1 in plan:
            v = volumes[s0:s1] if volumes.is_cuda else volumes[s0:s1].to(dev)
            if fused:
                xs = nn_common.preprocess_volumes(v, rescale, mode=mode)
            else:
                feat = common.process_volumes(v, mode=mode, scale=False)
                xs = nn_common.preprocess_features(feat, dims, rescale, out_dtype="bfloat16")
            out[s0:s1] = self._forward_timed(xs, trunk_events)

    def _chain_slices(self, volumes, plan, out, rescale, exact_resize, trunk_events, ijk, T):
        """:meth:`_chain_serial` on target slices: ``T`` rows per frame, ``ijk`` (N,3) / (N,T,3) or None (derived targets).  Returns the
        (N,T,3) int32 CUDA indices the rows were sliced at.  Grids and rescales the fused preprocessing does not take, and
        ``exact_resize``: float32 slice rows (``process_volumes``) and the Pillow-exact resize, the same rows."""
        import torch
        from . import common, nn_common
        dims = tuple(int(v) for v in volumes.shape[1:])
        dev = out.device
        fused = not exact_resize and nn_common.preprocess_supported(dims, rescale)
        used = []
        for s0, s1 in plan:
            v = volumes[s0:s1] if volumes.is_cuda else volumes[s0:s1].to(dev)
            idx = None if ijk is None else ijk[s0:s1]
            if fused:
                xs, got = nn_common.preprocess_volumes(v, rescale, mode="slice", ijk=idx, num_targets=T, return_ijk=True)
            else:
                feat, got = common.process_volumes(v, mode="slice", ijk=idx, num_targets=T, scale=False, return_ijk=True)
                xs = nn_common.preprocess_features(feat, dims, rescale, out_dtype="bfloat16")
            out[s0 * T:s1 * T] = self._forward_timed(xs, trunk_events)
            used.append(got)
        return used[0] if len(used) == 1 else torch.cat(used)

    def _chain_two_streams(self, volumes, plan, out, rescale, mode, trunk_events):
        """The ``overlap`` chain: the projection of pass b+2 on a second stream beside the resize of pass b+1, the trunk (a whole CU's
        LDS) and the dense tail (hipBLASLt: 135 KB of LDS) alone between two projection launches.  Measured in round 4 (three
        schedules, kernel timeline in tools/exp/README.md): no gain -- beside the projection the resize kernels take 3 x as long
        (both live on the LDS pipe and the issue ports) and the projection 1.25 x, so the pair costs what the two cost in turn:
        4.6-4.7 against 4.7-4.8 M frames/s."""
        import torch
        from . import common, nn_common, _lib
        dims = tuple(int(v) for v in volumes.shape[1:])
        dev, nb, bs = out.device, len(plan), plan[0][1]
        lib, ctx = _lib.load(), _lib.context(dev)
        cur = torch.cuda.current_stream(dev)
        sp = getattr(self, "_proj_stream", None)
        if sp is None or sp.device != dev:
            sp = self._proj_stream = torch.cuda.Stream(device=dev)
        feats = [torch.empty((bs, common.feature_len(*dims)), dtype=torch.float32, device=dev) for _ in range(2)]
        ev_proj = [torch.cuda.Event(), torch.cuda.Event()]
        sp.wait_stream(cur)                         # the volumes (and the fresh buffers) are the caller's stream's
        _lib.check(lib.rml_ctx_set_option(ctx, _lib.OPT_PROJECT_SHARE_CU, 1), "rml_ctx_set_option")
        ev_trunk = [torch.cuda.Event(), torch.cuda.Event()]
        try:
            def project(b):
                k, (s0, s1) = b & 1, plan[b]
                with torch.cuda.stream(sp):
                    if b >= 2:
                        # not before the trunk of batch b-2 is done: the trunk needs a whole CU's LDS, and a projection launch
                        # that reaches the CUs first keeps it waiting (two persistent kernels taking turns CU by CU: measured
                        # slower than one stream).  That trunk is also behind the resizes that read this buffer.
                        sp.wait_event(ev_trunk[k])
                    common.process_volumes(volumes[s0:s1], mode=mode, scale=False, out=feats[k][:s1 - s0])
                    ev_proj[k].record(sp)

            def resize(b):
                k, (s0, s1) = b & 1, plan[b]
                cur.wait_event(ev_proj[k])
                return nn_common.preprocess_features(feats[k][:s1 - s0], dims, rescale, out_dtype="bfloat16")
            project(0)
            project(1)
            xs = resize(0)
            for b, (s0, s1) in enumerate(plan):
                if b + 1 < nb:
                    cur.wait_event(ev_proj[(b + 1) & 1])    # the trunk could not start beside the running projection anyway
                fv = self._features_timed(xs, trunk_events)
                ev_trunk[b & 1].record(cur)
                if b + 2 < nb:
                    project(b + 2)                  # second stream: behind this trunk
                if b + 1 < nb:
                    xs = resize(b + 1)              # float64 VALU work beside the streaming projection of batch b+2
                # the dense tail last: hipBLASLt's kernel wants 135 KB of LDS and waits for the projection to leave the CUs
                out[s0:s1] = self.dense_tail(fv)
        finally:
            _lib.check(lib.rml_ctx_set_option(ctx, _lib.OPT_PROJECT_SHARE_CU, 0), "rml_ctx_set_option")
        cur.wait_stream(sp)

    # ---- margin guard: float64 labels from a bf16 chain (dnn_guard.py) -----------------------------------------
    _gaps = staticmethod(dnn_guard.top2_gaps)

    @property
    def last_guard(self):
        """What the last guarded call did (the keys: dnn_guard.py)."""
        return self._margin.last

    def _guard(self, proba, eps, rescore):
        """Replace the rows of ``proba`` (N, C) whose top-2 gap is below ``eps`` -- too small for a bf16 chain -- by what
        ``rescore(rows, precision)`` gives from exact inputs: dnn_guard.MarginGuard (the policy: rounds, stages "x3" -> "x6" ->
        "float64", the self-calibrating gap, remembered per weight version) on dnn_guard.CudaOps (csrc/guard.hip)."""
        return self._margin.run(proba, eps, rescore, dnn_guard.CudaOps(), self.parameters())

    # ---- exact-input arithmetic: what the guard re-scores with -------------------------------------------------
    def x3_supported(self, H, W):
        """True when csrc/dnn_x3.hip takes (H, W) planes of this model: three branches of Conv2D(1->64) -> Conv2D(64->32), 3x3."""
        from . import _lib
        return (len(self.branches) == 3 and all(tuple(br[0].conv.weight.shape) == (64, 1, 3, 3) and tuple(br[1].conv.weight.shape) == (32, 64, 3, 3)
                                                for br in self.branches)
                and bool(_lib.load().rml_dnn_trunk_x3_supported(int(H), int(W))))

    def features_x3(self, xz, yz, xy, parts=2):
        """The conv features in float32 from the float32-class trunk (csrc/dnn_x3.hip): (N,H,W) or (N,1,H,W) CUDA float32 planes ->
        (N, 38 400) rows in Keras' Flatten order.  ``parts`` = 2: ~2^-16 relative per product (bf16 pairs, three matrix-core
        products each, "x3"); 3: ~2^-24 (bf16 triples, six products, "x6")."""
        import torch
        from . import _lib
        lib = _lib.load()
        xs = [x.reshape(x.shape[0], x.shape[-2], x.shape[-1]).float().contiguous() for x in (xz, yz, xy)]
        n, H, W = xs[0].shape
        dev = xs[0].device
        w1, b1, w2, b2 = self._conv_packs()["x3"]
        feat = torch.empty((n, (H // 4) * (W // 4) * 96), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rml_dnn_trunk_x3(_lib.context(dev), _lib.ptr(xs[0]), _lib.ptr(xs[1]), _lib.ptr(xs[2]), n, H, W, _lib.ptr(w1),
                                            _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), int(parts), _lib.ptr(feat), _lib.stream_ptr(dev)), "rml_dnn_trunk_x3")
        return feat

    def forward_exact(self, xz, yz, xy, precision="float64"):
        """The layers of dnn.py:45-91 on the inputs' device with no single-bf16 operand anywhere, dropout inactive whatever the
        module's mode: (N,H,W) or (N,1,H,W) planes -> (N, n_classes) probabilities.
        "x3" / "x6": the float32-class HIP trunk (:meth:`features_x3`, two / three bf16 parts per operand) + the dense layers in
        float32 (:meth:`_tail_float32`) -- the margin guard's first two stages; planes it does not take fall to "float32".
        "float32": the plain PyTorch layers (MIOpen float32 convolutions, hipBLASLt), the reference's own arithmetic.  "float64": im2col
        by nine strided slices + rocBLAS matrix products (MIOpen has no float64 convolution and PyTorch's fallback takes 10 ms for a
        handful of rows; F.unfold is as slow)."""
        import torch
        import torch.nn.functional as F
        if precision not in ("x3", "x6", "float32", "float64"):
            raise ValueError("precision must be 'x3', 'x6', 'float32' or 'float64'")
        if precision != "float64":
            with torch.autocast("cuda", enabled=False):
                xs = [x.reshape(x.shape[0], 1, x.shape[-2], x.shape[-1]).float() for x in (xz, yz, xy)]
                if precision in ("x3", "x6") and xs[0].is_cuda and self.x3_supported(xs[0].shape[-2], xs[0].shape[-1]):
                    fv = self.features_x3(*xs, parts=3 if precision == "x6" else 2)
                else:
                    fv = self.features(*xs)
                return self._tail_float32(fv)
        dt = torch.float64
        w = self._exact_weights(dt)
        outs = []
        for x, convs in zip((xz, yz, xy), w["conv"]):
            x = x.reshape(x.shape[0], 1, x.shape[-2], x.shape[-1]).to(dt)
            for (k2d, b, kh, kw) in convs:
                ph, pw = tf_same_pad(x.shape[-2], kh, 2), tf_same_pad(x.shape[-1], kw, 2)
                oh, ow = -(-x.shape[-2] // 2), -(-x.shape[-1] // 2)
                xp = F.pad(x, (pw[0], pw[1], ph[0], ph[1]))
                # (N, Cin, kh*kw, oh, ow) -> (N, Cin*kh*kw, oh*ow): the (cin, ky, kx) order of weight.reshape(Cout, -1)
                cols = torch.stack([xp[:, :, ky:ky + 2 * oh - 1:2, kx:kx + 2 * ow - 1:2] for ky in range(kh) for kx in range(kw)], dim=2)
                cols = cols.reshape(x.shape[0], -1, oh * ow)
                x = F.relu(torch.matmul(k2d, cols) + b[None, :, None]).reshape(x.shape[0], k2d.shape[0], oh, ow)
            outs.append(x)
        h = flatten_nhwc(torch.cat(outs, dim=1))
        (w1, b1), (w2, b2), (w3, b3) = w["fc"]
        # the first dense layer as a batch of K-slices: rocBLAS' float64 GEMM with a few rows and K = 38 400 runs on a handful of
        # workgroups (6 ms for 32 rows); 150 slices of 256 in one batched call and a sum take 0.1 ms
        K = int(h.shape[1])
        kc = 256 if K % 256 == 0 else K
        part = torch.bmm(h.reshape(h.shape[0], K // kc, kc).transpose(0, 1), w1.reshape(w1.shape[0], K // kc, kc).permute(1, 2, 0))
        h = F.relu(part.sum(dim=0) + b1)
        h = F.relu(F.linear(h, w2, b2))
        return torch.softmax(F.linear(h, w3, b3), dim=-1)

    def forward_float64(self, xz, yz, xy):
        """:meth:`forward_exact` in float64: what the oracle's NumPy restatement computes, to ~1e-16."""
        return self.forward_exact(xz, yz, xy, "float64")

    def exact_features(self, volumes, rows=None, rescale=(80, 80), mode="max", parts=2):
        """CUDA volumes (float32 or uint8) -> float32-class conv features of frames ``rows`` (an int64 CUDA index tensor; None:
        all) in ONE library call (rml_dnn_exact_features: gather, exact projection, Pillow-bit-identical resize, x3 / x6 trunk)."""
        import torch
        from . import _lib, common
        lib = _lib.load()
        v, vdt = common._as_device_volumes(volumes)
        dev = v.device
        X, Y, Z = (int(t) for t in v.shape[1:])
        n = int(rows.numel()) if rows is not None else int(v.shape[0])
        oh, ow = int(rescale[1]), int(rescale[0])
        w1, b1, w2, b2 = self._conv_packs()["x3"]
        feat = torch.empty((n, (oh // 4) * (ow // 4) * 96), dtype=torch.float32, device=dev)
        if n == 0:
            return feat
        if rows is not None:
            rows = rows.to(device=dev, dtype=torch.int64).contiguous()
        nbytes = int(lib.rml_dnn_exact_features_scratch_bytes(vdt, n, X, Y, Z, oh, ow, 1 if rows is not None else 0))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rml_dnn_exact_features(_lib.context(dev), _lib.ptr(v), vdt, _lib.ptr(rows), n, X, Y, Z, _lib.MODES[mode], oh, ow,
                                                  _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), int(parts), _lib.ptr(scratch), nbytes,
                                                  _lib.ptr(feat), _lib.stream_ptr(dev)), "rml_dnn_exact_features")
        return feat

    def rescore_exact(self, volumes, rescale=(80, 80), mode="max", precision="float64", rows=None, ijk=None):
        """(n,X,Y,Z) volumes -> (n, n_classes) probabilities through the reference's chain without a rounding the reference does
        not have: projection (exact), (p - 127.5) / 127.5 and Pillow's bicubic resize in float64 rounded to float32 planes as
        Pillow stores them (csrc/resize.hip, bit-identical), then the layers in ``precision`` (:meth:`forward_exact`: "x3",
        "float32" -- the reference's own arithmetic, dnn.py runs Keras in float32 -- or "float64", the oracle's).  ``rows``: an index
        tensor -- score ``volumes[rows]`` (in that order), a pass of at most RESCORE_BYTES of volumes at a time.  A sparse ``rows``
        gathers its frames (:func:`rescore_route`: in one library call per pass where that takes them); when at least half of the
        frames are wanted the passes project whole contiguous blocks of frames instead (no 480 KB-per-frame gather) and pick the
        40 KB feature rows.

        ``mode="slice"``: ``ijk`` (n,3) or (n,T,3) -- the result has n*T rows, frame-major, and ``rows`` indexes THOSE: row r is scored
        from frame r // T at ijk[r] (``nn_common.slice_row_targets``), through ``process_volumes(mode="slice", ijk=...)`` (exact), the
        Pillow-exact resize and :meth:`forward_exact`.  The passes themselves: dnn_guard.ExactRescore."""
        return self._rescore(volumes, rescale, mode, precision, rows, ijk)

    def _one_call_route(self, volumes, rescale, mode, precision):
        import torch
        return (precision in ("x3", "x6") and volumes.is_cuda and mode != "slice" and self.x3_supported(int(rescale[1]), int(rescale[0]))
                and volumes.dtype in (torch.float32, torch.uint8) and volumes.is_contiguous())

    def _one_call(self, volumes, rows, rescale, mode, precision):
        return self._tail_float32(self.exact_features(volumes, rows, rescale, mode, 3 if precision == "x6" else 2))

    # ---- training (dnn.py:89-90, 347-390) ------------------------------------------------------------------------
    def compile(self, lr=0.0002, beta_1=0.5, beta_2=0.999, epsilon=1e-7, seed=0):
        """Keras ``model.compile(optimizer=Adam(lr=0.0002, beta_1=0.5), loss='sparse_categorical_crossentropy')`` (dnn.py:89-90): a fresh
        optimizer state (nn_common.DeviceAdam: torch.optim.Adam's form, epsilon inside the bias-corrected denominator where Keras adds it
        outside).  ``seed`` seeds the dropout masks and the epoch permutations.  ``fit`` / ``train_on_batch`` imply it with these
        defaults."""
        self._opt = {"lr": float(lr), "beta_1": float(beta_1), "beta_2": float(beta_2), "epsilon": float(epsilon), "seed": int(seed)}
        self._adam, self._grads, self._train_steps = None, None, 0
        self._rng = np.random.default_rng(int(seed))
        return self

    def _job(self, x, y, validation_data, class_weight, batch_size, trusted):
        if self._opt is None:
            self.compile()
        if len(x) != 3:
            raise ValueError("expected the three inputs [xz, yz, xy]")
        xs = [_planes(a) for a in x]
        y = _labels(y)
        if any(a.shape != xs[0].shape for a in xs) or len(y) != len(xs[0]) or len(y) == 0:
            raise ValueError("fit: three equal plane sets and one label per sample expected")
        if trusted and (y.min() < 0 or y.max() >= self.n_classes):
            raise ValueError("fit: labels outside [0, %d)" % self.n_classes)
        val_xs = val_y = None
        if validation_data is not None:
            val_xs = [_planes(a) for a in validation_data[0]]
            val_y = _labels(validation_data[1])
            if len(val_xs) != 3 or any(a.shape[1:] != xs[0].shape[1:] or len(a) != len(val_y) for a in val_xs) or len(val_y) == 0:
                raise ValueError("fit: validation_data = ([xz, yz, xy], y) with the training planes' shape expected")
            if val_y.min() < 0 or val_y.max() >= self.n_classes:
                raise ValueError("fit: validation labels outside [0, %d)" % self.n_classes)
            val_y = val_y.astype(np.int32)
        return FitJob(xs, y.astype(np.int32), val_xs, val_y, _class_weights(class_weight, self.n_classes), batch_size, self.drop.p,
                      self._opt["seed"], trusted)

    def train_on_batch(self, x, y, class_weight=None):
        """Keras ``model.train_on_batch([xz, yz, xy], y, class_weight=...)``: one update on these samples (at most 64); returns
        (loss, accuracy) of the batch in train mode, before the update."""
        job = self._job(x, y, None, class_weight, len(_labels(y)), trusted=False)
        n = len(job.y)
        ls, co, _, _ = _fit_epoch(self, job, np.arange(n, dtype=np.int32))
        return ls / n, co / n

    def fit(self, x, y, batch_size=64, epochs=100, validation_data=None, class_weight=None, shuffle=True, patience=None, checkpoint=None):
        """Keras ``model.fit`` as dnn.py:373-381 calls it.  ``x`` = [xz, yz, xy] planes, (N,H,W) or (N,H,W,1), already scaled to [-1, 1];
        ``validation_data`` = ([xz, yz, xy], y).  The data set is uploaded once; every epoch draws a permutation from the NumPy generator
        that ``compile(seed=...)`` seeded and reads device memory once.  ``patience``: EarlyStopping(monitor='val_loss', patience) -- training
        stops when val_loss has not been below its best for ``patience`` epochs, the model keeps its LAST weights; ``checkpoint``: a path
        that receives ``state_dict()`` whenever val_loss improves (ModelCheckpoint(save_best_only=True)).  Returns a :class:`History`:
        loss / accuracy are the train-mode running means of the epoch (sum of weighted losses / N, correct / N), val_loss / val_accuracy
        the eval-mode means (unweighted, as Keras)."""
        import torch
        if (patience is not None or checkpoint is not None) and validation_data is None:
            raise ValueError("fit: patience and checkpoint monitor val_loss: validation_data is needed")
        job = self._job(x, y, validation_data, class_weight, batch_size, trusted=True)
        n = len(job.y)
        hist = History(validation_data is not None)
        best = wait = None
        for ep in range(int(epochs)):
            perm = self._rng.permutation(n) if shuffle else np.arange(n)
            ls, co, vls, vco = _fit_epoch(self, job, perm.astype(np.int32))
            hist.epoch.append(ep)
            hist.history["loss"].append(ls / n)
            hist.history["accuracy"].append(co / n)
            if validation_data is None:
                continue
            val_loss = vls / len(job.val_y)
            hist.history["val_loss"].append(val_loss)
            hist.history["val_accuracy"].append(vco / len(job.val_y))
            if best is None or val_loss < best:
                best, wait = val_loss, 0
                if checkpoint is not None:
                    torch.save(self.state_dict(), checkpoint)
            else:
                wait += 1
                if patience is not None and wait >= patience:
                    hist.stopped_epoch = ep
                    break
        return hist

    # ---- Keras surface -----------------------------------------------------------------------------------------
    def predict(self, inputs, batch_size=8192, autocast_dtype="bfloat16", label_guard=LABEL_GUARD, fused=None):
        """Keras ``model.predict([xz, yz, xy])``: numpy (N,H,W,1) inputs -> (N, n_classes) float32 numpy.  Under autocast on the
        GPU the margin guard of :meth:`predict_volumes` applies: rows whose top-2 gap is below ``label_guard`` are scored again
        in float64 from the same input planes, so ``argmax`` is the float64 label.  ``fused`` (default: where the planes fit the
        fused kernels -- the 80 x 80 of dnn.py do -- and the dtype is bfloat16): the bf16 chain of :meth:`predict_volumes`
        (csrc/dnn.hip trunk + csrc/dense.hip tail) instead of the PyTorch / MIOpen layers under autocast -- the same operand
        precision, one launch per stage: dnn.py:373-381 predicts ONE target per call (round 6)."""
        import torch
        dev = next(self.parameters()).device
        dt = getattr(torch, autocast_dtype) if autocast_dtype else None
        was = self.training
        self.eval()
        outs = []
        n = len(inputs[0])
        with torch.no_grad():
            for s in range(0, n, batch_size):
                xs = [to_nchw(a[s:s + batch_size], dev) for a in inputs]
                H, W = int(xs[0].shape[-2]), int(xs[0].shape[-1])
                reduced = dt is not None and dev.type == "cuda"            # a reduced-precision chain: guarded
                use_fused = (fused if fused is not None else True) and dt is torch.bfloat16 and dev.type == "cuda" \
                    and all(tuple(x.shape[-2:]) == (H, W) and x.shape[1] == 1 for x in xs) and self.kblock_supported(H, W) and self.x3_supported(H, W)
                if use_fused:
                    p = self.forward_fused(*xs)
                elif reduced:
                    with torch.autocast("cuda", dtype=dt):
                        p = self(*xs)
                else:
                    p = self(*xs)
                if reduced:
                    p = self._guard(p.float(), label_guard, lambda idx, prec: self.forward_exact(*[x[idx] for x in xs], precision=prec))
                outs.append(p.float().cpu())
        self.train(was)
        return torch.cat(outs).numpy() if outs else np.zeros((0, self.n_classes), np.float32)
