"""Shared pieces of the SGAN inference tests: the test model (weights redrawn so that an indexing mistake shows), the planes, the plain
PyTorch inference path (float32, or under autocast) and the tolerance yardstick -- the plain path under bf16 autocast against the plain
path in float32, same weights, same planes, measured at run time over a fixed case set."""
import contextlib
import functools
import importlib

import numpy as np

SLOPE = 0.2
# (H, W, batch, classes, seed): the sizes of the trunk tests (fewer samples than waves, odd batches, more than one workgroup round),
# the default size, the end-to-end cases
YARDSTICK_CASES = ((8, 8, 33, 3, 1), (16, 16, 33, 3, 2), (16, 40, 33, 3, 3), (40, 16, 33, 3, 4), (128, 128, 9, 3, 5), (128, 128, 5, 5, 6),
                   (16, 16, 7, 3, 7))


def sgan_module():
    return importlib.import_module("radar_ml_amd.sgan")


def make_model(H, W, C, seed, device="cpu", dtype=None):
    """Discriminator at (H, W) planes with weights that make mistakes visible: the N(0, 0.02) init gives near-uniform probabilities
    that hide an indexing error.  Kernels ~ N(0, gain / sqrt(fan_in)) (gain sqrt(2) in front of a LeakyReLU keeps the activations
    O(1); the last layer's is larger so that the probabilities are decided), biases ~ N(0, 0.2), BatchNorm gamma in [0.5, 1.5], beta
    and moving mean ~ N(0, 0.3), moving variance in [0.5, 2]."""
    import torch
    sgan = sgan_module()
    g = torch.Generator().manual_seed(1000 + seed)
    m = sgan.Discriminator(((H, W, 1),) * 3, C)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
                fan_in = mod.weight[0].numel()
                gain = 6.0 if mod is m.fc3 else 2.0 ** 0.5
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (gain / fan_in ** 0.5))
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
            elif isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.3)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 1.5 + 0.5)
    if dtype is not None:
        m = m.to(dtype)
    return m.to(device).eval()


def make_planes(B, H, W, seed, device="cpu", dtype=None):
    """three (B, H, W) plane sets uniform in [-1, 1]; non-zero in the first and last rows and columns, so a symmetric pad instead of
    TensorFlow's (0, 1) is caught"""
    import torch
    g = torch.Generator().manual_seed(2000 + seed)
    xs = [torch.rand((B, H, W), generator=g) * 2.0 - 1.0 for _ in range(3)]
    for x in xs:
        assert bool((x[:, 0] != 0).all()) and bool((x[:, -1] != 0).all()) and bool((x[:, :, 0] != 0).all()) and bool((x[:, :, -1] != 0).all())
    return [x.to(device=device, dtype=dtype or torch.float32) for x in xs]


def plain_eval(model, xs, autocast=None):
    """``Discriminator.forward`` in inference mode on the plain PyTorch layers, with the flattened trunk output handed back too:
    (features (N, K), probabilities (N, C)), both float32 (float64 for a float64 model).  ``autocast``: a CUDA autocast dtype."""
    import torch
    from radar_ml_amd.nn_common import flatten_nhwc
    model.eval()
    dt = next(model.parameters()).dtype
    x4 = [x.reshape(x.shape[0], 1, x.shape[-2], x.shape[-1]).to(dt) for x in xs]
    ctx = torch.autocast("cuda", dtype=autocast) if autocast is not None else contextlib.nullcontext()
    with torch.no_grad(), ctx:
        fv = flatten_nhwc(torch.cat([br(x) for x, br in zip(x4, model.branches)], dim=1))
        h = model.act(model.bn1(model.fc1(fv)))
        h = model.act(model.bn2(model.fc2(h)))
        lg = model.fc3(h)
    out = torch.float64 if dt == torch.float64 else torch.float32
    return fv.to(out), torch.softmax(lg.to(out), dim=-1)


def folded_eval(folded, xs):
    """the model of ``sgan.fold_batchnorm`` applied with plain F.conv2d / F.linear: (features, logits)"""
    import torch
    import torch.nn.functional as F
    from radar_ml_amd.nn_common import flatten_nhwc
    slope = folded["slope"]
    outs = []
    for x, layers in zip(xs, folded["conv"]):
        h = x.reshape(x.shape[0], 1, x.shape[-2], x.shape[-1]).to(layers[0][0].dtype)
        for w, b in layers:
            h = F.leaky_relu(F.conv2d(F.pad(h, (0, 1, 0, 1)), w, b, stride=2), slope)       # even sizes: 'same' pads bottom / right
        outs.append(h)
    fv = flatten_nhwc(torch.cat(outs, dim=1))
    (w1, b1), (w2, b2), (w3, b3) = folded["fc"]
    h = F.leaky_relu(F.linear(fv, w1, b1), slope)
    h = F.leaky_relu(F.linear(h, w2, b2), slope)
    return fv, F.linear(h, w3, b3)


def feat_error(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.double() - ref.double()).abs().max()) / float(ref.double().abs().max())


@functools.lru_cache(maxsize=None)
def case(H, W, B, C, seed):
    """(model on the GPU, planes, float32 features, float32 probabilities) of one case, computed once and shared"""
    model = make_model(H, W, C, seed, device="cuda")
    xs = make_planes(B, H, W, seed, device="cuda")
    fv, p = plain_eval(model, xs)
    return model, xs, fv, p


@functools.lru_cache(maxsize=None)
def yardstick():
    """(E_feat, E_p): what bf16 autocast costs the plain PyTorch inference path against the same path in float32, the largest
    over YARDSTICK_CASES.  Also asserts that the float32 probabilities of the case set are decided (largest probability above 0.5 on
    most rows), so that a comparison of probabilities means something."""
    import torch
    e_feat = e_p = 0.0
    decided = rows = 0
    for c in YARDSTICK_CASES:
        model, xs, fv, p = case(*c)
        fv16, p16 = plain_eval(model, xs, autocast=torch.bfloat16)
        e_feat = max(e_feat, feat_error(fv16, fv))
        e_p = max(e_p, float((p16 - p).abs().max()))
        decided += int((p.max(dim=1).values > 0.5).sum())
        rows += int(p.shape[0])
    print("yardstick (plain eval, bf16 autocast against float32): E_feat = %.3e, E_p = %.3e; %d of %d rows decided" % (e_feat, e_p, decided, rows))
    assert decided >= 0.7 * rows, "the test models give near-uniform probabilities (%d of %d rows above 0.5)" % (decided, rows)
    assert 0.0 < e_feat < 0.1 and 0.0 < e_p < 0.5
    return e_feat, e_p


def check_labels(p_fused, p_ref, e_p, what):
    """every row whose float32 top-2 gap exceeds 2 * (2 * E_p) has the float32 label; rows under that gap are counted and reported"""
    import torch
    top2 = p_ref.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    clear = gap > 4.0 * e_p
    near = int((~clear).sum())
    print("%s: %d of %d rows within the near-tie gap %.2e (not asserted)" % (what, near, int(p_ref.shape[0]), 4.0 * e_p))
    assert torch.equal(p_fused.argmax(dim=1)[clear], p_ref.argmax(dim=1)[clear])
    return near


def synth_frames(n, grid, seed):
    """n radar frames of integer returns in [0, 255] on ``grid`` (float32 numpy), from the project's synthetic source"""
    import oracle_np as O
    vol, _ = O.synth_volumes(seed, n, *grid)
    assert np.array_equal(vol, np.round(vol)) and vol.min() >= 0 and vol.max() <= 255
    return vol.astype(np.float32)
