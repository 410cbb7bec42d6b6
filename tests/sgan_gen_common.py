"""NumPy float64 twin of one branch of the SGAN generator, written from the layer formulas (no torch): Dense -> ReLU -> NHWC
reshape -> n_up x [Conv2DTranspose(4x4, stride 2, 'same') in scatter form + BatchNormalization + ReLU] -> Conv2D(1, 7x7, 'same')
+ tanh.  Weights in the Keras layouts of ``Generator.keras_weights()``."""
import numpy as np

BN_EPS = 1e-3


def conv_transpose_scatter(x, K, b):
    """x (n, H, W, ci), Keras kernel K (4, 4, co, ci): every input pixel (iy, ix) is scattered to the output pixels
    oy = 2 iy + ky - 1, ox = 2 ix + kx - 1 that fall inside the (2H, 2W) output."""
    n, H, W, _ = x.shape
    co = K.shape[2]
    out = np.zeros((n, 2 * H, 2 * W, co), np.float64)
    iys, ixs = np.arange(H), np.arange(W)
    for ky in range(4):
        oys = 2 * iys + ky - 1
        my = (oys >= 0) & (oys < 2 * H)
        for kx in range(4):
            oxs = 2 * ixs + kx - 1
            mx = (oxs >= 0) & (oxs < 2 * W)
            contrib = np.einsum("nhwi,oi->nhwo", x, K[ky, kx])
            out[:, oys[my][:, None], oxs[mx][None, :], :] += contrib[:, iys[my][:, None], ixs[mx][None, :], :]
    return out + b


def conv7_same(x, k, b):
    """x (n, H, W, c), Keras kernel k (7, 7, c, 1), zero padding 3 on every side -> (n, H, W, 1)"""
    n, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (3, 3), (3, 3), (0, 0)))
    out = np.zeros((n, H, W), np.float64)
    for ky in range(7):
        for kx in range(7):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ k[ky, kx, :, 0]
    return out[..., None] + b


def twin_branch(z, weights, base, training):
    """(n, S, S, 1) output of one branch; ``weights`` = one entry of ``Generator.keras_weights()``"""
    (dk, db), ups, (ok, ob) = weights
    z = np.asarray(z, np.float64)
    ch = ups[0][0].shape[3] if ups else ok.shape[2]
    h = np.maximum(z @ dk + db, 0.0).reshape(z.shape[0], base, base, ch)        # unit j = (h * base + w) * ch + c
    for K, b, gamma, beta, mean, var in ups:
        o = conv_transpose_scatter(h, K, b)
        if training:
            mean, var = o.mean(axis=(0, 1, 2)), o.var(axis=(0, 1, 2))
        h = np.maximum((o - mean) / np.sqrt(var + BN_EPS) * gamma + beta, 0.0)
    return np.tanh(conv7_same(h, ok, ob))


def random_keras_weights(model, rng, scale=0.3):
    """non-trivial weights, biases and moving statistics in the layouts (and shapes) of ``model.keras_weights()``"""
    out = []
    for dense, ups, outc in model.keras_weights():
        new_ups = []
        for K, b, g, be, mu, var in ups:
            new_ups.append((rng.normal(0, scale, K.shape), rng.normal(0, 0.2, b.shape), rng.uniform(0.5, 1.5, g.shape),
                            rng.normal(0, 0.3, be.shape), rng.normal(0, 0.5, mu.shape), rng.uniform(0.5, 2.0, var.shape)))
        out.append([(rng.normal(0, scale, dense[0].shape), rng.normal(0, 0.2, dense[1].shape)), new_ups,
                    (rng.normal(0, scale, outc[0].shape), rng.normal(0, 0.2, outc[1].shape))])
    return out


# ---- whole g step: gradients of one path against another (GPU tests and the measurement behind their tolerances) ---------------

def gan_param_class(name):
    """'g.branches.B.ups.I.weight' -> 'g.up.kernel' ...; 'd.branches.B.{1,4,7}.weight' -> 'd.bn1/2/3.gamma' ...: the classes the
    tolerances are kept per (all branches and all up-sampling layers of a kind together)"""
    parts = name.split(".")
    kind = {"weight": "gamma", "bias": "beta"}
    if parts[0] == "g":
        layer = parts[3]
        if layer == "dense":
            return "g.dense." + ("kernel" if parts[-1] == "weight" else "bias")
        if layer == "ups":
            return "g.up%s." % parts[4] + ("kernel" if parts[-1] == "weight" else "bias")
        if layer == "bns":
            return "g.bn%s." % parts[4] + kind[parts[-1]]
        return "g.out." + ("kernel" if parts[-1] == "weight" else "bias")
    if parts[1] == "branches":
        return "d.bn%d.%s" % (int(parts[3]) // 3 + 1, kind[parts[-1]])
    return "d.dense_%s.%s" % (parts[1], kind[parts[-1]])


def g_step_gradients(sgan, gen, disc, z, y, amp, plain, scale=256.0):
    """(loss, {parameter name: gradient}) of one ``GanTrainer`` step's loss without the update: ``amp`` None = float32, else the
    autocast type with a fixed loss scale; ``plain`` = the plain PyTorch layers instead of the fused ones."""
    import contextlib
    dt = sgan.DiscriminatorTrainer(disc, amp_dtype=amp, ddp=False)
    if dt._scale_t is not None:
        dt._scale_t.fill_(scale)
    gan = sgan.GanTrainer(gen, dt)
    with (sgan.plain_layers() if plain else contextlib.nullcontext()):
        loss, grads = gan.gradients(z, y)
    div = scale if dt._scale_t is not None else 1.0
    return float(loss), {k: (None if g is None else g.detach().float() / div) for k, g in zip(gan.param_names, grads)}


def grad_rel_errors(g_ref, g_test):
    """worst |test - ref| / |ref| per parameter class; parameters without gradient in both are skipped"""
    worst = {}
    for k, a in g_ref.items():
        b = g_test[k]
        if a is None or b is None:
            assert a is None and (b is None or float(b.abs().max()) == 0.0), k
            continue
        na = float(a.norm())
        assert na > 0.0, k
        rel = float((b - a).norm()) / na
        cls = gan_param_class(k)
        worst[cls] = max(worst.get(cls, 0.0), rel)
    return worst


def gan_pair(sgan, size, seed=11):
    """(generator, discriminator, z, y) on the GPU at the reduced ('small': n_up 1, 16 x 16, batch 4) or the default size (batch 2),
    dropout off, non-trivial biases in front of the batch norms"""
    import torch
    torch.manual_seed(seed)
    if size == "small":
        gen = sgan.Generator(latent_dim=100, channels=128, base=8, n_up=1).to("cuda").to(memory_format=torch.channels_last)
        disc = sgan.Discriminator(((16, 16, 1),) * 3, 3).to("cuda").to(memory_format=torch.channels_last)
        n = 4
    else:
        gen, disc, n = sgan.define_generator(device="cuda"), sgan.define_discriminator(device="cuda"), 2
    disc.drop.p = 0.0
    with torch.no_grad():
        for mod in list(gen.modules()) + list(disc.modules()):
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                mod.bias.normal_(0.0, 0.05)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    z = torch.randn((n, 100), device="cuda", generator=g)
    y = torch.rand((n, 1), device="cuda", generator=g) * 0.5 + 0.7
    return gen, disc, z, y
