"""Shared pieces of the generator-inference tests: the test generator (weights redrawn so that an indexing mistake shows), a float64
NumPy twin of the fused chain that consumes the PACKED layouts of ``rml_sgan_generate`` and computes the transposed convolution by
output phases (with the mutations the CPU tests need), the plain PyTorch inference path and the tolerance yardstick -- the plain path
under half-precision autocast against the plain path in float32, measured at run time over the case set."""
import contextlib
import functools
import importlib

import numpy as np

from sgan_gen_common import conv7_same

BN_EPS = 1e-3
# gains of the redrawn kernels (std = gain / sqrt(fan_in)): sqrt(2) in front of a ReLU keeps the activations O(1); the output layer's
# is chosen so that the float32 images are neither flat nor saturated (test_gen_infer_cpu.test_images_are_neither_flat_nor_saturated)
GAIN_RELU = 2.0 ** 0.5
GAIN_OUT = 0.6
# (latent_dim, channels, base, n_up, batch, seed): the whole-chain cases of the GPU tests
CHAIN_CASES = tuple((16, 128, 8, n_up, B, 10 * n_up + B) for n_up in (1, 2) for B in (1, 3, 9)) + ((100, 128, 8, 4, 2, 51), (100, 128, 8, 4, 5, 52))


def sgan_module():
    return importlib.import_module("radar_ml_amd.sgan")


def make_generator(latent_dim, channels, base, n_up, seed, device="cpu", dtype=None):
    """Generator with weights that make mistakes visible (the N(0, 0.02) init gives images near 0 that hide an indexing error):
    kernels ~ N(0, gain / sqrt(fan_in)) -- fan_in of a transposed convolution: the 2x2 taps an output pixel meets times the input
    channels --, biases ~ N(0, 0.2), BatchNorm gamma in [0.5, 1.5], beta and moving mean ~ N(0, 0.3), moving variance in [0.5, 2]."""
    import torch
    sgan = sgan_module()
    g = torch.Generator().manual_seed(3000 + seed)
    m = sgan.Generator(latent_dim=latent_dim, channels=channels, base=base, n_up=n_up)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.Linear):
                fan_in, gain = mod.in_features, GAIN_RELU
            elif isinstance(mod, torch.nn.ConvTranspose2d):
                fan_in, gain = 4 * mod.in_channels, GAIN_RELU
            elif isinstance(mod, torch.nn.Conv2d):
                fan_in, gain = 49 * mod.in_channels, GAIN_OUT
            elif isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.3)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 1.5 + 0.5)
                continue
            else:
                continue
            mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (gain / fan_in ** 0.5))
            mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
    if dtype is not None:
        m = m.to(dtype)
    return m.to(device).to(memory_format=torch.channels_last).eval()


def make_latent(B, latent_dim, seed, device="cpu", dtype=None):
    import torch
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.randn((B, latent_dim), generator=g).to(device=device, dtype=dtype or torch.float32)


def plain_eval(model, z, autocast=None):
    """The plain PyTorch layers in inference mode, called directly (not through ``Generator.forward``): three (n, 1, S, S) tensors,
    float32 (float64 for a float64 model).  ``autocast``: a CUDA autocast dtype."""
    import torch
    import torch.nn.functional as F
    model.eval()
    par = next(model.parameters())
    z = z.to(device=par.device, dtype=par.dtype)
    ctx = torch.autocast("cuda", dtype=autocast) if autocast is not None else contextlib.nullcontext()
    outs = []
    with torch.no_grad(), ctx:
        for br in model.branches:
            h = F.relu(br.dense(z)).reshape(z.shape[0], model.base, model.base, model.channels).permute(0, 3, 1, 2)
            for up, bn in zip(br.ups, br.bns):
                h = F.relu(bn(up(h)))
            outs.append(torch.tanh(br.out(h)).to(torch.float64 if par.dtype == torch.float64 else torch.float32))
    return outs


# ---- the float64 twin ---------------------------------------------------------------------------------------------------------------
MUTATIONS = ("ky", "halo", "phases", "bias_mu")


def twin_pack_up(w, mutation=None):
    """folded Keras kernel w (4, 4, co, ci) -> wt (4, co, 4 ci): wt[p*2+q][co][(a*2+b)*ci_n + ci] = w[ky][kx][co][ci] with
    ky = 3 - p - 2a, kx = 3 - q - 2b.  Mutation 'ky': ky = p + 2a."""
    co, ci = w.shape[2], w.shape[3]
    wt = np.zeros((4, co, 4 * ci), np.float64)
    for p in (0, 1):
        for q in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    ky = p + 2 * a if mutation == "ky" else 3 - p - 2 * a
                    kx = 3 - q - 2 * b
                    wt[p * 2 + q][:, (a * 2 + b) * ci:(a * 2 + b + 1) * ci] = w[ky, kx]
    return wt


def twin_packs(keras_weights, mutation=None):
    """``Generator.keras_weights()`` -> the packed float64 arrays of ``rml_sgan_generate``, folded here in NumPy: s = gamma /
    sqrt(var + eps), w' = K s[co], b' = beta + (b - mean) s.  Mutation 'bias_mu': b' = beta + b s."""
    dw, db, uw, ub, ow, ob = [], [], [], [], [], []
    for (dk, dbias), ups, (ok, obias) in keras_weights:
        dw.append(np.asarray(dk, np.float64)); db.append(np.asarray(dbias, np.float64))
        lw, lb = [], []
        for K, b, gamma, beta, mean, var in ups:
            s = gamma / np.sqrt(var + BN_EPS)
            lw.append(twin_pack_up(K * s[None, None, :, None], mutation))
            lb.append(beta + (b if mutation == "bias_mu" else b - mean) * s)
        uw.append(np.stack(lw)); ub.append(np.stack(lb))
        ow.append(np.asarray(ok, np.float64).reshape(49, -1)); ob.append(float(np.asarray(obias).reshape(())))
    return {"dense_w": np.stack(dw), "dense_b": np.stack(db), "up_wt": np.stack(uw), "up_bias": np.stack(ub), "out_w": np.stack(ow),
            "out_b": np.asarray(ob, np.float64)}


def twin_up_linear(x, wt, bias, mutation=None):
    """bias + the four phase GEMMs, before the ReLU.  x (n, H, W, C), wt (4, co, 4 C), bias (co) -> (n, 2H, 2W, co): output pixel
    (2m+p, 2n+q) reads the window rows m-1+p+a, columns n-1+q+b (zeros outside the plane).  Mutations: 'halo' puts the zero halo
    on the other side (rows m+p+a, columns n+q+b), 'phases' stores phase (p, q) where (q, p) belongs."""
    n, H, W, C = x.shape
    co = wt.shape[1]
    pad = ((0, 0), (0, 2), (0, 2), (0, 0)) if mutation == "halo" else ((0, 0), (1, 1), (1, 1), (0, 0))
    xp = np.pad(x, pad)                                    # xp[:, iy + 1] = x[:, iy]
    out = np.zeros((n, 2 * H, 2 * W, co), np.float64)
    for p in (0, 1):
        for q in (0, 1):
            acc = np.zeros((n, H, W, co), np.float64)
            for a in (0, 1):
                for b in (0, 1):
                    win = xp[:, p + a:p + a + H, q + b:q + b + W, :]
                    acc += win @ wt[p * 2 + q][:, (a * 2 + b) * C:(a * 2 + b + 1) * C].T
            if mutation == "phases":
                out[:, q::2, p::2] = acc + bias
            else:
                out[:, p::2, q::2] = acc + bias
    return out


def twin_up(x, wt, bias, mutation=None):
    return np.maximum(twin_up_linear(x, wt, bias, mutation), 0.0)


def twin_generate(z, packs, base, mutation=None):
    """three (n, S, S) float64 images from the packed arrays (NumPy, any float type)"""
    z = np.asarray(z, np.float64)
    C = packs["out_w"].shape[-1]
    outs = []
    for br in range(3):
        h = np.maximum(z @ np.asarray(packs["dense_w"][br], np.float64) + np.asarray(packs["dense_b"][br], np.float64), 0.0)
        h = h.reshape(z.shape[0], base, base, C)
        for l in range(packs["up_wt"].shape[1]):
            h = twin_up(h, np.asarray(packs["up_wt"][br, l], np.float64), np.asarray(packs["up_bias"][br, l], np.float64), mutation)
        k = np.asarray(packs["out_w"][br], np.float64).reshape(7, 7, C, 1)
        outs.append(np.tanh(conv7_same(h, k, float(packs["out_b"][br])))[..., 0])
    return outs


def packs_numpy(pk):
    return {k: v.detach().double().cpu().numpy() for k, v in pk.items()}


# ---- GPU cases and the yardstick --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(latent_dim, channels, base, n_up, B, seed):
    """(model on the GPU, latent points, float32 images of the plain layers) of one case, computed once and shared"""
    model = make_generator(latent_dim, channels, base, n_up, seed, device="cuda")
    z = make_latent(B, latent_dim, seed, device="cuda")
    return model, z, plain_eval(model, z)


def image_error(got, ref):
    """max |got - ref| over the three images (they live in [-1, 1])"""
    return max(float((g.double() - r.double()).abs().max()) for g, r in zip(got, ref))


def in_band(images, lo=0.05, hi=0.95):
    """smallest fraction, over the three images, of pixels with lo <= |v| <= hi"""
    return min(float(((v.abs() >= lo) & (v.abs() <= hi)).double().mean()) for v in images)


@functools.lru_cache(maxsize=None)
def yardstick(dtype_name):
    """what autocast of ``dtype_name`` costs the plain PyTorch layers against the same layers in float32: the largest image error
    over CHAIN_CASES"""
    import torch
    adt = getattr(torch, dtype_name)
    e = 0.0
    for c in CHAIN_CASES:
        model, z, ref = case(*c)
        e = max(e, image_error(plain_eval(model, z, autocast=adt), ref))
    print("yardstick (plain eval, %s autocast against float32): E = %.3e" % (dtype_name, e))
    assert 0.0 < e < 0.5
    return e
