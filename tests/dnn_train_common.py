"""Shared by test_dnn_train_cpu.py / test_dnn_train_gpu.py: the case grid of the CNN training step, its float64 / float32
PyTorch-CPU autograd restatement (the "twin"), and a direct driver of rml_dnn_train_step.

The twin restates radar-ml_amd/csrc/dnn_train.hip from include/radarml.h: TF 'same' padding (bottom / right), NHWC flatten, dropout
masks from the library's own host function rml_dnn_dropout_mask, the class-weighted softmax cross-entropy summed over the batch and
divided by B, torch.optim.Adam's update.  In float64 it is the reference; the same code in float32 is the yardstick for rounding.

Cases sit on a grid where the convolution trunk is exact in float32 in any summation order (relu masks cannot flip):
inputs multiples of 1/4 in [-1, 0.75] with ~60 % of the pixels at -1; conv1 kernels multiples of 1/16 in [-1/4, 1/4], biases odd
multiples of 1/128 up to 17/128; conv2 kernels multiples of 1/32 in [-1/8, 1/8], biases odd multiples of 2^-13 up to 129/8192.  The dense
layers keep Glorot weights; a case takes the first seed of 0..7 whose float64 dense pre-activations are all >= 1e-4 from zero."""
import contextlib
import ctypes
import functools

import numpy as np

# (H, W, B, C)
SHAPES = [(8, 8, 1, 3), (8, 8, 5, 2), (12, 20, 3, 5), (20, 12, 7, 3), (80, 80, 3, 3), (80, 80, 37, 3), (80, 80, 64, 3)]
RATES = (0.5, 0.0)
CLASS_WEIGHTS = (1.0, 1.26, 5.48, 2.0, 0.5)        # the first three: the reference's train.log
EXTRA_ROWS = 5                                      # resident samples beyond the batch
SEED, STEP = 1234, 7                                # dropout seed and step of the single-step cases
DENSE_MARGIN = 1e-4
TRUNK_MARGIN = 2.0 ** -13
ADAM = dict(lr=0.0002, beta_1=0.5, beta_2=0.999, epsilon=1e-7)


def lib():
    from radar_ml_amd import _lib
    return _lib.load()


def keep_mask(seed, step, layer, B, rate, n_units=64):
    """(B, n_units) uint8 of rml_dnn_dropout_mask: 1 = kept"""
    out = np.empty((B, n_units), np.uint8)
    L = lib()
    for b in range(B):
        rc = L.rml_dnn_dropout_mask(int(seed), int(step), int(layer), b, n_units, float(rate), out[b].ctypes.data)
        assert rc == 0
    return out


def keep_scale(rate):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
def twin_features(params, xs, dtype):
    """(B, K) features of planes xs = three (B, H, W) tensors; params: the module's 18 tensors"""
    import torch
    import torch.nn.functional as F
    outs = []
    for br in range(3):
        k1, b1, k2, b2 = params[4 * br:4 * br + 4]
        x = xs[br].to(dtype).unsqueeze(1)
        x = F.relu(F.conv2d(F.pad(x, (0, 1, 0, 1)), k1, b1, stride=2))          # even sizes, stride 2, 3x3: pad bottom / right
        x = F.relu(F.conv2d(F.pad(x, (0, 1, 0, 1)), k2, b2, stride=2))
        outs.append(x)
    x = torch.cat(outs, dim=1)
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)


def twin_step(params, xs, y, rows, cw, seed, step, rate, dtype, train=True):
    """One step of the restatement on the batch ``rows`` of resident planes ``xs`` (three (N, H, W) arrays) / labels ``y``.
    Returns dict(loss_sum, correct, grads (train), z1, z2): loss_sum = sum_b w_b l_b, the gradients those of loss_sum / B."""
    import torch
    import torch.nn.functional as F
    rows = np.asarray(rows, dtype=np.int64)
    B = len(rows)
    ps = [p.detach().cpu().to(dtype).contiguous().clone().requires_grad_(train) for p in params]
    xb = [torch.from_numpy(np.ascontiguousarray(a[rows])) for a in xs]
    yb = torch.from_numpy(np.asarray(y)[rows].astype(np.int64))
    w = torch.ones(len(yb), dtype=dtype) if cw is None else torch.from_numpy(np.asarray(cw, dtype=np.float64))[yb].to(dtype)
    with torch.set_grad_enabled(train):
        fv = twin_features(ps, xb, dtype)
        z1 = F.linear(fv, ps[12], ps[13])
        h = F.relu(z1)
        if train:
            h = h * torch.from_numpy(keep_mask(seed, step, 0, B, rate).astype(np.float64) * keep_scale(rate)).to(dtype)
        z2 = F.linear(h, ps[14], ps[15])
        h = F.relu(z2)
        if train:
            h = h * torch.from_numpy(keep_mask(seed, step, 1, B, rate).astype(np.float64) * keep_scale(rate)).to(dtype)
        z3 = F.linear(h, ps[16], ps[17])
        lb = w * (torch.logsumexp(z3, dim=1) - z3[torch.arange(B), yb])
        loss_sum = lb.sum()
        if train:
            (loss_sum / B).backward()
    return {"loss_sum": float(loss_sum.detach()), "correct": int((z3.argmax(dim=1) == yb).sum()), "grads": [p.grad for p in ps] if train else None,
            "z1": z1.detach(), "z2": z2.detach()}


class TwinTrainer:
    """The restatement of ``dnn._fit_epoch`` in ``dtype`` on the CPU: same signature once bound (``trainer(model, job, perm)``), keeps
    its own parameters (from the model at the first call) and torch.optim.Adam, and writes the trained values back into the model."""

    def __init__(self, dtype):
        self.dtype, self.params, self.opt, self.steps = dtype, None, None, 0
        self.perms = []

    def __call__(self, model, job, perm):
        import torch
        o = model._opt
        if self.params is None:
            self.params = [p.detach().cpu().to(self.dtype).contiguous().clone() for p in model.parameters()]
            self.opt = torch.optim.Adam(self.params, lr=o["lr"], betas=(o["beta_1"], o["beta_2"]), eps=o["epsilon"])
        self.perms.append(np.array(perm))
        ls, co = 0.0, 0
        for off in range(0, len(perm), job.batch_size):
            r = twin_step(self.params, job.xs, job.y, perm[off:off + job.batch_size], job.class_weight, job.seed, self.steps, job.rate, self.dtype)
            for p, g in zip(self.params, r["grads"]):
                p.grad = g
            self.opt.step()
            self.steps += 1
            ls += r["loss_sum"]
            co += r["correct"]
        vls, vco = 0.0, 0
        if job.val_xs is not None:
            r = twin_step(self.params, job.val_xs, job.val_y, np.arange(len(job.val_y)), None, 0, 0, 0.0, self.dtype, train=False)
            vls, vco = r["loss_sum"], r["correct"]
        with torch.no_grad():
            for p, q in zip(model.parameters(), self.params):
                p.copy_(q.to(device=p.device, dtype=p.dtype))
        model._train_steps = self.steps
        return ls, co, vls, vco


@contextlib.contextmanager
def hooked(D, fn):
    """``dnn._fit_epoch`` replaced by ``fn`` inside the block"""
    old = D._fit_epoch
    D._fit_epoch = fn
    try:
        yield
    finally:
        D._fit_epoch = old


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def grid_planes(rng, n, H, W):
    """three (n, H, W) float32 plane sets on the input grid"""
    out = []
    for _ in range(3):
        v = rng.integers(-4, 4, size=(n, H, W)).astype(np.float32) / 4.0
        v[rng.random((n, H, W)) < 0.6] = -1.0
        out.append(v)
    return out


def grid_trunk_(model, rng):
    """put the convolution parameters of ``model`` on the weight grid (in place)"""
    import torch
    with torch.no_grad():
        for br in model.branches:
            c1, c2 = br[0].conv, br[1].conv
            c1.weight.copy_(torch.from_numpy(rng.integers(-4, 5, size=tuple(c1.weight.shape)) / 16.0))
            c1.bias.copy_(torch.from_numpy((2 * rng.integers(-9, 9, size=64) + 1) / 128.0))
            c2.weight.copy_(torch.from_numpy(rng.integers(-4, 5, size=tuple(c2.weight.shape)) / 32.0))
            c2.bias.copy_(torch.from_numpy((2 * rng.integers(-65, 65, size=32) + 1) / 8192.0))
    return model


def make_model(H, W, C, seed, device="cpu"):
    """define_classifier on ``device``: Glorot dense layers drawn under torch seed ``seed``, the trunk on the grid (one draw per shape)"""
    import torch
    from radar_ml_amd import dnn as D
    torch.manual_seed(seed)
    m = D.define_classifier((H, W, 1), (H, W, 1), (H, W, 1), n_classes=C, device="cpu")
    grid_trunk_(m, np.random.default_rng(1000 + 7 * H + W))
    return m.to(device) if device != "cpu" else m


def dense_preactivations(params, fv, B, rate):
    """float64 z1, z2 of the two hidden dense layers on features ``fv`` in train mode at (SEED, STEP, rate)"""
    import torch
    import torch.nn.functional as F
    W1, b1, W2, b2 = (p.detach().double() for p in params[12:16])
    z1 = F.linear(fv, W1, b1)
    h = F.relu(z1) * torch.from_numpy(keep_mask(SEED, STEP, 0, B, rate).astype(np.float64) * keep_scale(rate))
    return z1, F.linear(h, W2, b2)


def draw(H, W, B, C):
    rng = np.random.default_rng(H * 1000003 + W * 1009 + B * 17 + C)
    N = B + EXTRA_ROWS
    xs = grid_planes(rng, N, H, W)
    y = rng.integers(0, C, size=N).astype(np.int32)
    rows = rng.permutation(N)[:B].astype(np.int32)
    return xs, y, rows


def dense_seed(H, W, B, C, xs, rows):
    """the first seed of 0..7 whose float64 dense pre-activations all have |z| >= DENSE_MARGIN at both rates, or None"""
    import torch
    fv = None
    for seed in range(8):
        params = list(make_model(H, W, C, seed).parameters())
        if fv is None:                      # the trunk does not depend on the seed
            with torch.no_grad():
                fv = twin_features([p.detach().double() for p in params], [torch.from_numpy(a[rows.astype(np.int64)]) for a in xs], torch.float64)
        if all(float(z.abs().min()) >= DENSE_MARGIN for rate in RATES for z in dense_preactivations(params, fv, B, rate)):
            return seed
    return None


@functools.lru_cache(maxsize=None)
def case(H, W, B, C):
    """dict: model seed, resident planes xs / labels y (N = B + EXTRA_ROWS), rows, class weights cw, and per rate the float64 and
    float32 twin steps ("t64", "t32")"""
    import torch
    xs, y, rows = draw(H, W, B, C)
    cw = np.asarray(CLASS_WEIGHTS[:C], dtype=np.float32)
    seed = dense_seed(H, W, B, C, xs, rows)
    if seed is None:
        raise AssertionError("no seed of 0..7 keeps the dense pre-activations of case %s %g from zero" % ((H, W, B, C), DENSE_MARGIN))
    params = list(make_model(H, W, C, seed).parameters())
    t64 = {rate: twin_step(params, xs, y, rows, cw, SEED, STEP, rate, torch.float64) for rate in RATES}
    t32 = {rate: twin_step(params, xs, y, rows, cw, SEED, STEP, rate, torch.float32) for rate in RATES}
    return {"seed": seed, "xs": xs, "y": y, "rows": rows, "cw": cw, "t64": t64, "t32": t32, "shape": (H, W, B, C)}


def grad_errors(grads, grads64):
    """e = max|g - g64| / max|g64| per parameter tensor"""
    return [float((g.detach().cpu().double() - r).abs().max() / r.abs().max()) for g, r in zip(grads, grads64)]


@functools.lru_cache(maxsize=None)
def e32():
    """E32: the largest gradient error the float32 CPU twin shows against the float64 one over all cases and both rates"""
    return max(max(grad_errors(case(*s)["t32"][r]["grads"], case(*s)["t64"][r]["grads"])) for s in SHAPES for r in RATES)


# ---- the device step, called directly -------------------------------------------------------------------------------------------
GUARD = 12345.0


class DeviceStep:
    """rml_dnn_train_step on the parameters of a CUDA ``model``: gradients, accumulators and status live inside one buffer filled with
    GUARD, 64 guard floats around each of them (``guards_intact``)."""

    def __init__(self, model, xs, y, cw):
        import torch
        from radar_ml_amd import _lib, dnn as D
        self._lib, self.model = _lib, model
        self.params = list(model.parameters())
        dev = self.dev = self.params[0].device
        self.x = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in xs]
        self.y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(dev)
        self.cw = None if cw is None else torch.from_numpy(np.asarray(cw, dtype=np.float32)).to(dev)
        self.N, self.H, self.W = (int(v) for v in self.x[0].shape)
        self.layout = D._k2_layout(self.params)
        sizes = [p.numel() for p in self.params] + [8]           # the last: loss sum (double) | correct | status | 4 spare ints
        offs, o = [], 64
        for n in sizes:
            offs.append(o)
            o += ((n + 63) // 64) * 64 + 64
        self.buf = torch.full((o,), GUARD, dtype=torch.float32, device=dev)
        self.inside = torch.zeros((o,), dtype=torch.bool, device=dev)
        for at, n in zip(offs, sizes):
            self.inside[at:at + n] = True
        self.grads = [self.buf[at:at + p.numel()].as_strided(tuple(p.shape), tuple(p.stride())) for at, p in zip(offs, self.params)]
        self.acc = self.buf[offs[-1]:offs[-1] + 8]

    def run(self, rows, seed, step, rate, mode, B=None):
        """returns (loss_sum, correct, status); the gradients are in self.grads"""
        import torch
        _lib = self._lib
        L = _lib.load()
        rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.dev)
        B = len(rows) if B is None else B
        nbytes = int(L.rml_dnn_train_workspace_bytes(B, self.H, self.W, self.model.n_classes))
        assert nbytes > 0
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.dev)
        self.acc.view(torch.int32).zero_()
        pp = (ctypes.c_void_p * 18)(*[p.data_ptr() for p in self.params])
        gp = (ctypes.c_void_p * 18)(*[g.data_ptr() for g in self.grads])
        a0 = self.acc.data_ptr()
        with torch.cuda.device(self.dev):
            _lib.check(L.rml_dnn_train_step(_lib.context(self.dev), _lib.ptr(self.x[0]), _lib.ptr(self.x[1]), _lib.ptr(self.x[2]), _lib.ptr(self.y),
                                            _lib.ptr(rows_t), B, self.N, self.H, self.W, _lib.ptr(self.cw), self.model.n_classes, pp, gp, self.layout,
                                            seed, step, rate, mode, _lib.ptr(ws), nbytes, ctypes.c_void_p(a0), ctypes.c_void_p(a0 + 8),
                                            ctypes.c_void_p(a0 + 12), _lib.stream_ptr(self.dev)), "rml_dnn_train_step")
            torch.cuda.synchronize(self.dev)
        host = self.acc.cpu()
        return float(host.view(torch.float64)[0]), int(host.view(torch.int32)[2]), int(host.view(torch.int32)[3])

    def guards_intact(self):
        return bool((self.buf[~self.inside] == GUARD).all())

