"""Float64 twins, derived error bounds and the case table for the sweep of csrc/bnact.hip and csrc/optim.hip (NumPy only; shared by
test_bnact_cpu.py, which shows that twins and cases are fit to judge a kernel, and test_bnact_gpu.py, which judges the kernels).

Layout: activations are NHWC arrays (N, H, W, C), images (N, 2H+1, 2W+1), first-layer weights [tap = ky * 3 + kx][C].  Every twin
takes inputs that were already rounded to the kernel's input format (half activations, float32 parameters and hyper-parameters)
and widened to float64; nothing inside a twin is rounded.

Bounds (u = 2^-24; all first-order, hence the factor 4 on each):
  L          longest float32 summation chain of the kernel: pixels per thread + lanes added up afterwards (chain_* below)
  e_r        (L + 2) u (1 + d^2 / (var + eps)), d = |pivot - mean|: relative error of rstd from sums of (x - pivot), (x - pivot)^2
             (q/M - (s/M)^2 = var with q/M = var + d^2, (s/M)^2 = d^2, each off by L u of its size).  The same sums put the mean off
             by L u (|d| + sigma) <= e_r sqrt(2 (var + eps)) -- an error relative to the channel's spread, which is what z sees; so the
             bound on save_mean is 4 e_r max(|mean|, sqrt(var + eps)): relative to the mean where that is the larger of the two.
  tau        16 u (|x - mean| rstd |gamma| + |mean| rstd |gamma| + |beta|): rounding of z itself (the first layer adds its nine FMAs,
             sum_k |w_k t_k| rstd |gamma|).  |z| < tau: the kernel may sit on the other side of the LeakyReLU kink (mask).
  y, dx      0.5 ulp_half + 4 (float32 error of the value before it is rounded); the ulp is taken at |reference| + that error, since
             the kernel rounds its own float32 value, which may lie in the next binade
  running    momentum * (bound of the batch statistic) + u |new value| (the result is a float32 the kernel rounds once more)
The first layer's statistics come from 54 image sums without a pivot: conv1_bounds derives their error from the sums of absolute
taps and tap products instead (e_m for the mean, e_r for rstd)."""
import numpy as np

U = 2.0 ** -24
HALF = {"float16": (11, -14), "bfloat16": (8, -126)}        # significand bits (hidden one included), exponent of the smallest normal
EPS, MOMENTUM = 1e-3, 0.01
EPS32, MOM32 = float(np.float32(EPS)), float(np.float32(MOMENTUM))      # as the C ABI's float arguments carry them


# ---- number formats ------------------------------------------------------------------------------------------------------------
def to_bits(a, kind):
    """round float values to the half type `kind` (nearest even): uint16 bit patterns"""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    if kind == "float16":
        return a32.astype(np.float16).view(np.uint16)
    b = a32.view(np.uint32).astype(np.uint64)
    nan = np.isnan(a32)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    b = np.where(nan, 0x7FC0, b)
    return b.astype(np.uint16)


def from_bits(b, kind):
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if kind == "float16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def round_half(a, kind):
    return from_bits(to_bits(a, kind), kind)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def ulp_h(v, kind):
    """spacing of the half type at v, floored at the smallest normal"""
    p, emin = HALF[kind]
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** emin))      # |v| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - p)


def ulp32(v):
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -126))
    return np.ldexp(1.0, e - 24)


# ---- launch geometry (stats_grid and the launchers of bnact.hip) --------------------------------------------------------------------
def stats_grid(M, C, num_cu):
    PL = 256 // (C // 8)
    return max(1, min((M + PL - 1) // PL, 8 * num_cu))


def chain_bn(M, C, num_cu):
    """k_bn_stats / k_bn_bwd_reduce: pixels per thread + the PL pixel lanes block_channel_sums adds"""
    PL = 256 // (C // 8)
    return -(-M // (stats_grid(M, C, num_cu) * PL)) + PL


def chain_imgstats(M, num_cu):
    """k_c1_imgstats: pixels per thread + six DPP levels + four waves"""
    GI = max(1, min(8 * num_cu, (M + 255) // 256))
    return -(-M // (GI * 256)) + 6 + 4


def chain_c1_bwd(N, H, W, C, num_cu, packed):
    """k_c1_bwd1 / k_c1_bwd1_pk: rows per workgroup * pixels per thread and row + the pixel lanes.  The packed kernel runs one round
    of resident workgroups: at least one per CU, which bounds the chain from above."""
    G = stats_grid(N * H * W, C, num_cu)
    if packed:
        G = min(G, num_cu)
    cpt = 4 if (C % 4 == 0 and 256 % (C // 4) == 0 and C // 4 <= 256) else 8
    PL = 256 // (C // cpt)
    return -(-(N * H) // G) * -(-W // PL) + PL


def takes_packed(C, W):
    return C == 128 and W in (16, 32, 64)


# ---- BatchNorm + LeakyReLU + pad ------------------------------------------------------------------------------------------------------
def bn_forward(x, gamma, beta, eps, momentum, slope, ph, pw, running_mean, running_var, mutation=None):
    N, H, W, C = x.shape
    M = N * H * W
    xs = x.reshape(M, C)
    if mutation == "drop_last":
        xs = xs[:-1]
    mean = xs.mean(0)
    mean = mean + (xs - mean).mean(0)
    var = ((xs - mean) ** 2).mean(0)                     # two-pass
    Ms = xs.shape[0]
    nvar = var * Ms / (Ms - 1) if mutation == "unbiased_var" else var
    rstd = 1.0 / np.sqrt(nvar + eps)
    ga = np.roll(gamma, 1) if mutation == "roll_gamma" else gamma
    xc = x - mean
    xh = xc * rstd
    z = xh * ga + beta
    pos = z >= 0 if mutation == "ge_zero" else z > 0
    y = np.zeros((N, H + ph, W + pw, C))
    y[:, :H, :W] = np.where(pos, z, z * slope)
    tau = 16 * U * (np.abs(xc) * rstd * np.abs(gamma) + np.abs(mean) * rstd * np.abs(gamma) + np.abs(beta))
    unb = M / (M - 1.0) if M > 1 else 1.0
    return dict(z=z, y=y, mean=mean, var=var, rstd=rstd, xh=xh, pos=pos, tau=tau, mask=np.abs(z) < tau,
                running_mean=(1 - momentum) * running_mean + momentum * mean,
                running_var=(1 - momentum) * running_var + momentum * var * unb)


def bn_backward(x, dy_padded, gamma, beta, eps, slope, ph, pw, mutation=None):
    """reads only the unpadded part of dy"""
    N, H, W, C = x.shape
    M = N * H * W
    f = bn_forward(x, gamma, beta, eps, 0.0, slope, 0, 0, np.zeros(C), np.ones(C), mutation if mutation in ("ge_zero", "roll_gamma") else None)
    if mutation == "roll_gamma":
        gamma = np.roll(gamma, 1)
    dy = dy_padded[:, ph:ph + H, :W] if mutation == "pad_from_dy" else dy_padded[:, :H, :W]
    g = np.where(f["pos"], dy, dy * slope)
    dbeta = g.reshape(M, C).sum(0)
    dgamma = (g * f["xh"]).reshape(M, C).sum(0)
    c1, c2 = dbeta / M, dgamma / (M - 1 if mutation == "c2_m1" else M)
    dx = gamma * f["rstd"] * (g - c1 - f["xh"] * c2)
    return dict(g=g, dx=dx, dgamma=dgamma, dbeta=dbeta, c1=c1, c2=c2, dy=dy)


def bn_bounds(x, gamma, beta, eps, momentum, slope, f, b, L, kind):
    """bound of every output of the two entry points for one case (f, b: the twins' results; L: chain_bn)"""
    N, H, W, C = x.shape
    M = N * H * W
    d = np.abs(x[0, 0, 0] - f["mean"])
    e_r = (L + 2) * U * (1 + d * d / (f["var"] + eps))
    sd = np.sqrt(f["var"] + eps)
    out = dict(e_r=e_r)
    out["mean"] = 4 * e_r * np.maximum(np.abs(f["mean"]), sd)
    out["rstd"] = 4 * e_r * f["rstd"]
    unb = M / (M - 1.0) if M > 1 else 1.0
    out["running_mean"] = momentum * out["mean"] + U * np.abs(f["running_mean"])
    out["running_var"] = momentum * unb * 8 * e_r * (f["var"] + eps) + U * np.abs(f["running_var"])
    act_gain = np.where(f["pos"], 1.0, abs(slope))
    slack = 4 * act_gain * (f["tau"] + np.abs(f["xh"] * gamma) * e_r)
    out["y"] = 0.5 * ulp_h(np.abs(f["y"][:, :H, :W]) + slack, kind) + slack
    ag, agx = np.abs(b["g"]).reshape(M, C).sum(0), np.abs(b["g"] * f["xh"]).reshape(M, C).sum(0)
    slack = 4 * np.abs(gamma) * f["rstd"] * (4 * U * (np.abs(b["g"]) + np.abs(b["c1"]) + np.abs(f["xh"] * b["c2"]))
                                              + (L + 2) * U * (ag + np.abs(f["xh"]) * agx) / M)
    out["dx"] = 0.5 * ulp_h(np.abs(b["dx"]) + slack, kind) + slack
    kink_b, kink_g = kink_budget(f, b, slope)
    out["sum_dbeta"], out["sum_dgamma"] = 4 * (L + 2) * U * ag, 4 * (L + 2) * U * agx
    out["kink_dbeta"], out["kink_dgamma"] = kink_b, kink_g
    out["dbeta"], out["dgamma"] = out["sum_dbeta"] + kink_b, out["sum_dgamma"] + kink_g
    return out


def kink_budget(f, b, slope):
    """what the masked elements can move a channel's sum g and sum g x_hat by"""
    C = f["z"].shape[-1]
    m = f["mask"]
    return ((1 - slope) * (np.abs(b["dy"]) * m).reshape(-1, C).sum(0),
            (1 - slope) * (np.abs(b["dy"] * f["xh"]) * m).reshape(-1, C).sum(0))


# ---- the first layer: 3x3 stride-2 one-channel convolution folded in -------------------------------------------------------------------
def taps(img):
    H, W = (img.shape[1] - 1) // 2, (img.shape[2] - 1) // 2
    return np.stack([img[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] for ky in range(3) for kx in range(3)], -1)      # (N, H, W, 9)


def conv1_forward(img, w, gamma, beta, eps, momentum, slope, ph, pw, running_mean, running_var, mutation=None):
    """img: the already padded image; w [9][C]: the weights rounded to the half type, as Conv1BnLReluPad.forward rounds them"""
    t = taps(img)
    zc = t @ w
    f = bn_forward(zc, gamma, beta, eps, momentum, slope, ph, pw, running_mean, running_var, mutation)
    f["tau"] = f["tau"] + 16 * U * (np.abs(t) @ np.abs(w)) * f["rstd"] * np.abs(gamma)
    f["mask"] = np.abs(f["z"]) < f["tau"]
    f["t"], f["zc"] = t, zc
    return f


def conv1_backward(img, w, dy_padded, gamma, beta, eps, slope, ph, pw, mutation=None):
    t = taps(img)
    b = bn_backward(t @ w, dy_padded, gamma, beta, eps, slope, ph, pw, mutation)
    b["dW"] = np.einsum("nhwk,nhwc->kc", t, b["dx"])
    return b


def conv1_bounds(img, w, gamma, beta, eps, momentum, slope, f, b, Li, Lb, kind):
    """Li: chain_imgstats, Lb: chain_c1_bwd.  Statistics: mean = sum_j w_j B_j / M and E[z^2] = sum_jk w_j w_k T2_jk / M with every
    image sum off by (Li + 2) u of its sum of absolute terms."""
    t = f["t"]
    N, H, W, _ = t.shape
    C = w.shape[1]
    M = N * H * W
    ts = t.reshape(M, 9)
    at = np.abs(ts)
    S1, S2 = at.sum(0), at.T @ at                                  # sum |t_j|, sum |t_j t_k|
    B, T2 = ts.sum(0), ts.T @ ts
    aw = np.abs(w)
    a = (Li + 2) * U
    e_m = a * (S1 @ aw) / M + U * np.abs(f["mean"])
    e_var = a * np.einsum("jc,jk,kc->c", aw, S2, aw) / M + 2 * np.abs(f["mean"]) * e_m
    e_r = e_var / (2 * (f["var"] + eps)) + U
    out = dict(e_r=e_r, e_m=e_m)
    out["mean"], out["rstd"] = 4 * e_m, 4 * e_r * f["rstd"]
    unb = M / (M - 1.0) if M > 1 else 1.0
    out["running_mean"] = momentum * out["mean"] + U * np.abs(f["running_mean"])
    out["running_var"] = momentum * unb * 4 * e_var + U * np.abs(f["running_var"])
    act_gain = np.where(f["pos"], 1.0, abs(slope))
    slack = 4 * act_gain * (f["tau"] + np.abs(f["xh"] * gamma) * e_r + e_m * f["rstd"] * np.abs(gamma))
    out["y"] = 0.5 * ulp_h(np.abs(f["y"][:, :H, :W]) + slack, kind) + slack
    # the sums of the backward pass, each with its kink budget
    b_ = (Lb + 2) * U
    g = b["g"].reshape(M, C)
    ag, agx = np.abs(g).sum(0), np.abs(g * f["xh"].reshape(M, C)).sum(0)
    kink_b, kink_g = kink_budget(f, b, slope)
    mk = f["mask"].reshape(M, C) * np.abs(b["dy"].reshape(M, C))
    kink_A = (1 - slope) * (at.T @ mk)                             # [9][C]
    out["sum_dbeta"], out["sum_dgamma"] = 4 * b_ * ag, 4 * b_ * agx
    out["kink_dbeta"], out["kink_dgamma"] = kink_b, kink_g
    out["dbeta"], out["dgamma"] = out["sum_dbeta"] + kink_b, out["sum_dgamma"] + kink_g
    # dW = gamma rstd (A - c1 B - c2 D), D = rstd (sum_j w_j T2_jk - mean B_k): k_c1_wgrad_combine's expansion, term by term
    rs, mu = f["rstd"], f["mean"]
    dA = b_ * (at.T @ np.abs(g))
    dB, dT2 = a * S1, a * S2
    dc1, dc2 = b_ * ag / M, b_ * agx / M
    D = rs * (T2 @ w - np.outer(B, mu))                            # [9][C]
    dD = rs * (dT2 @ aw + np.outer(dB, np.abs(mu)))
    gr = np.abs(gamma) * rs
    out["sum_dW"] = 4 * (gr * (dA + np.outer(np.abs(B), dc1) + np.outer(dB, np.abs(b["c1"])) + np.abs(D) * dc2 + np.abs(b["c2"]) * dD)
                         + 4 * U * np.abs(b["dW"]))
    out["kink_dW"] = gr * (kink_A + np.outer(np.abs(B), kink_b / M) + np.abs(D) * kink_g / M)
    out["dW"] = out["sum_dW"] + out["kink_dW"]
    return out


# ---- Adam with the loss-scale rule ---------------------------------------------------------------------------------------------------
def adam_steps(p, grads, lr, betas, eps, scale, growth, backoff, interval, state=None, mutation=None):
    """torch.optim.Adam's formula (no weight decay, no amsgrad) + torch.amp.GradScaler's rule.  p: list of arrays; grads: per step a
    list of arrays (None: that parameter is left alone) as the optimizer receives them, i.e. multiplied by the current scale;
    scale None: no scaling and no test of the gradients.  state: dict(m, v, t, tracker) to continue from.  Returns one record per
    step: p, m, v (lists), t, scale, tracker, skipped, and upd = |the update of each element| / lr."""
    b1, b2 = betas
    p = [np.array(a, dtype=np.float64) for a in p]
    m = [np.zeros_like(a) for a in p] if state is None else [np.array(a, dtype=np.float64) for a in state["m"]]
    v = [np.zeros_like(a) for a in p] if state is None else [np.array(a, dtype=np.float64) for a in state["v"]]
    t, tracker = (0, 0) if state is None else (int(state["t"]), int(state["tracker"]))
    out = []
    for gs in grads:
        skipped = scale is not None and any(g is not None and not np.isfinite(g).all() for g in gs)
        inv = 1.0 if scale is None else 1.0 / scale
        upd = [np.zeros_like(a) for a in p]
        if scale is not None:
            if skipped:
                scale, tracker = scale * backoff, 0
            else:
                tracker += 1
                if tracker >= interval:
                    scale, tracker = scale * growth, 0
        if not skipped:
            t += 1
            tb = t - 1 if mutation == "bias_tm1" else t
            for i, g in enumerate(gs):
                if g is None:
                    continue
                gu = g * inv
                m[i] = b1 * m[i] + (1 - b1) * gu
                v[i] = b2 * v[i] + (1 - b2) * (g * g if mutation == "v_scaled" else gu * gu)
                bc1, bc2 = np.float64(1 - b1 ** tb), np.float64(1 - b2 ** tb)
                with np.errstate(divide="ignore", invalid="ignore"):
                    upd[i] = np.abs(m[i] / bc1) / (np.sqrt(v[i]) / np.sqrt(bc2) + eps)
                    p[i] = p[i] - (lr / bc1) * (m[i] / (np.sqrt(v[i]) / np.sqrt(bc2) + eps))
        out.append(dict(p=[a.copy() for a in p], m=[a.copy() for a in m], v=[a.copy() for a in v], t=t, scale=scale,
                        tracker=tracker, skipped=skipped, upd=upd))
    return out


def adam_update_condition(betas, t):
    """relative error of one update in units of u: the float32 operations of k_adam_apply (8) and its two bias corrections
    1 - powf(beta, t), whose cancellation multiplies powf's rounding by beta^t / (1 - beta^t) (2 ulps for bc1, half of 2 for the
    square root of bc2)"""
    b1, b2 = betas
    return 8 + 2 * b1 ** t / (1 - b1 ** t) + b2 ** t / (1 - b2 ** t)


def adam_p_bound(traj, p0, lr, betas):
    """|p_gpu - p_twin| after every step of a whole run: every step rounds p once (u |p|) and adds an update carrying the relative
    error above; first order, factor 4.  Returns per step a list of arrays."""
    acc = [np.zeros_like(np.asarray(a, dtype=np.float64)) for a in p0]
    out = []
    for r in traj:
        if not r["skipped"]:
            k = adam_update_condition(betas, r["t"])
            acc = [a + U * np.abs(pp) + U * lr * k * uu for a, pp, uu in zip(acc, r["p"], r["upd"])]
        out.append([4 * a for a in acc])
    return out


def adam_mv_bound(m_prev, v_prev, g_unscaled, betas, m_new, v_new):
    """one step from the kernel's own previous state: 2 float32 ulps.  v is a sum of non-negative terms: ulps of the result.  m may
    cancel (beta1 m and (1 - beta1) g of opposite sign), so its ulp is taken at |beta1 m| + |(1 - beta1) g|, which is |m_new|
    whenever nothing cancels."""
    b1, _ = betas
    return (2 * ulp32(np.abs(b1 * m_prev) + np.abs((1 - b1) * g_unscaled)), 2 * ulp32(v_new))


# ---- case tables -----------------------------------------------------------------------------------------------------------------
KINDS = ("float16", "bfloat16")
ALL_C = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)


def _bn(name, N, H, W, C, kind, slope=0.2, pad=(1, 1), abi=False, **kw):
    return dict(name="%s-%s" % (name, "h" if kind == "float16" else "b"), N=N, H=H, W=W, C=C, kind=kind, slope=slope, ph=pad[0], pw=pad[1],
                abi=abi or pad[0] != pad[1], **kw)


def bn_cases(num_cu):
    cap = 8 * num_cu
    cs = []
    for kind in KINDS:
        for C in ALL_C:                                   # M = 30: below PL for small C and no multiple of it; channel 0 is all zeros
            for slope in (0.2, 1.0):
                cs.append(_bn("c%d-s%g" % (C, slope), 2, 3, 5, C, kind, slope, zero_channel=True))
        for C in (8, 128):
            cs.append(_bn("one-c%d" % C, 1, 1, 1, C, kind, zero_channel=True))
        for C, N, W in ((2048, 1, None), (128, 2, 128), (8, 2, 512)):      # a second grid-stride iteration: M = cap PL + PL/2 + 1
            PL = 256 // (C // 8)
            M = cap * PL + PL // 2 + 1
            H, Wc = (1, M) if W is None else (-(-M // (N * W)), W)
            for slope in (0.2, 0.0):
                cs.append(_bn("stride2-c%d-s%g" % (C, slope), N, H, Wc, C, kind, slope, big=True))
        for C, W in ((128, 15), (128, 16), (8, 255), (8, 300)):            # Wp CG = 256, and past it by a non-multiple
            cs.append(_bn("rows-c%d-w%d" % (C, W), 3, 2, W, C, kind))
        for pad in ((0, 0), (1, 1), (0, 1), (1, 0)):                        # dy's pad row / column is NaN: never to be read
            cs.append(_bn("pad%d%d" % pad, 2, 3, 5, 16, kind, pad=pad, nan_pad=True))
    # ill-conditioned statistics: |mean| / std = 160 and 300 (no kink: slope 1); pixel 0 as a 4 sigma outlier moves the pivot
    for C in (8, 128):
        cs.append(_bn("ill-8-c%d" % C, 3, 25, 40, C, "float16", 1.0, ill=(8.0, 0.05)))
        cs.append(_bn("ill-30-c%d" % C, 3, 25, 40, C, "float16", 1.0, ill=(30.0, 0.1)))
        cs.append(_bn("ill-8-c%d" % C, 3, 25, 40, C, "bfloat16", 1.0, ill=(8.0, 0.25)))
    cs.append(_bn("ill-8-outlier-c8", 3, 25, 40, 8, "float16", 1.0, ill=(8.0, 0.05), outlier=4.0))
    for i, c in enumerate(cs):
        c["seed"] = 1000 + i
    return cs


def make_bn(c):
    """data of one case, already rounded: x, dy (padded), gamma, beta, running_mean, running_var.  Elements within 4 tau of the kink
    are moved away from it (the caps on masked elements are conditions on the case, see test_bnact_cpu.py)."""
    rng = np.random.default_rng(c["seed"])
    N, H, W, C, kind = c["N"], c["H"], c["W"], c["C"], c["kind"]
    if c.get("ill"):
        mu, sd = c["ill"]
        x = mu * np.where(np.arange(C) % 2 == 0, 1.0, -1.0) + sd * rng.standard_normal((N, H, W, C), dtype=np.float32)
        if c.get("outlier"):
            x[0, 0, 0] = mu * np.where(np.arange(C) % 2 == 0, 1.0, -1.0) + c["outlier"] * sd
    else:
        x = rng.standard_normal((N, H, W, C), dtype=np.float32) * 1.5 + rng.uniform(-1, 1, C).astype(np.float32)
    gamma = f32(rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.25, -1.0, 1.0))
    beta = f32(rng.uniform(-0.5, 0.5, C))
    if c.get("zero_channel"):
        x[..., 0] = 0.0
        beta[0] = 0.0
    x = round_half(x, kind)
    dy = round_half(rng.standard_normal((N, H + c["ph"], W + c["pw"], C), dtype=np.float32), kind)
    if c.get("nan_pad"):
        dy[:, H:] = np.nan
        dy[:, :, W:] = np.nan
    rm, rv = f32(rng.uniform(-0.5, 0.5, C)), f32(rng.uniform(0.5, 2.0, C))
    if c["slope"] != 1.0:
        for _ in range(8):
            f = bn_forward(x, gamma, beta, EPS32, MOM32, c["slope"], 0, 0, rm, rv)
            near = np.abs(f["z"]) < 4 * f["tau"]
            if not near.any():
                break
            x[near] = round_half(x[near] + 0.5, kind)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, running_mean=rm, running_var=rv)


def _c1(name, N, H, W, C, kind, sparse, slope=0.2, pad=(1, 1), **kw):
    return dict(name="%s-%s-%s" % (name, "sparse" if sparse else "dense", "h" if kind == "float16" else "b"), N=N, H=H, W=W, C=C,
                kind=kind, sparse=sparse, slope=slope, ph=pad[0], pw=pad[1], abi=pad[0] != pad[1], **kw)


# k_c1_bwd1 stages the three image rows of an output row, 3 (2 W + 1) floats, in its 2048 floats of LDS
C1_BWD_MAX_W = 340


def conv1_cases(num_cu):
    cs = []
    for kind in KINDS:
        for sparse in (False, True):
            cs.append(_c1("c2048", 1, 3, 3, 2048, kind, sparse))                     # k_c1_bwd1<., 8>
            for C in (8, 16, 64, 256, 1024):
                cs.append(_c1("c%d" % C, 2, 3, 5, C, kind, sparse))
            cs.append(_c1("c128-w8", 2, 5, 8, 128, kind, sparse))                   # general kernels; more rows than workgroups
            cs.append(_c1("c128-w72", 2, 5, 72, 128, kind, sparse))                 # longer than NB PL = 64: the reload branch
            cs.append(_c1("c1024-w9", 2, 3, 9, 1024, kind, sparse))                 # longer than NB PL = 8
            for W in (16, 32, 64):                                                  # the packed kernels (and the general ones)
                for H in (5, 16):
                    if H != W:
                        cs.append(_c1("pk-h%d-w%d" % (H, W), 2, H, W, 128, kind, sparse))
            # more rows than workgroups can be resident whatever the kernels' occupancy (at most 8 of 256 threads per CU)
            cs.append(_c1("pk-rows", max(100, 8 * num_cu // 16 + 1), 16, 16, 128, kind, sparse, big=True))
            for pad in ((0, 1), (1, 0)):
                cs.append(_c1("pad%d%d" % pad, 2, 3, 5, 16, kind, sparse, pad=pad, nan_pad=True))
        for C in (8, 64, 2048):
            cs.append(_c1("c%d-s1" % C, 2, 3, 5, C, kind, False, slope=1.0))
        # k_c1_imgstats' second iteration (M > 2048 * 256 at 256 CUs); rows this long are outside the backward's range
        Hs = -(-(8 * num_cu * 256 + 129) // (2 * 512))
        cs.append(_c1("imgstats2", 2, Hs, 512, 8, kind, False, big=True, fwd_only=True))
    for kind in KINDS:                                        # the longest row k_c1_bwd1 can stage: 3 (2 W + 1) = 2043 of 2048 floats
        cs.append(_c1("c8-w%d" % C1_BWD_MAX_W, 1, 2, C1_BWD_MAX_W, 8, kind, False))
    for i, c in enumerate(cs):
        c["seed"] = 5000 + i
    return cs


def make_conv1(c):
    """image (N, 2H+1, 2W+1) with its zero row and column, weights [9][C] rounded to the half type, dy, gamma, beta, running stats"""
    rng = np.random.default_rng(c["seed"])
    N, H, W, C, kind = c["N"], c["H"], c["W"], c["C"], c["kind"]
    raw = rng.uniform(-1, 1, (N, 2 * H, 2 * W)).astype(np.float32)
    if c["sparse"]:                                       # radar-like: background -1, 4 % returns
        raw = np.where(rng.random((N, 2 * H, 2 * W)) < 0.04, raw, np.float32(-1.0))
    img = np.zeros((N, 2 * H + 1, 2 * W + 1))
    img[:, :2 * H, :2 * W] = round_half(raw, kind)
    w = round_half(rng.normal(0, 0.3, (9, C)).astype(np.float32), kind)
    gamma = f32(rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.25, -1.0, 1.0))
    beta = f32(rng.uniform(-0.5, 0.5, C))
    dy = round_half(rng.standard_normal((N, H + c["ph"], W + c["pw"], C), dtype=np.float32), kind)
    if c.get("nan_pad"):
        dy[:, H:] = np.nan
        dy[:, :, W:] = np.nan
    rm, rv = f32(rng.uniform(-0.5, 0.5, C)), f32(rng.uniform(0.5, 2.0, C))
    if c["slope"] != 1.0:
        for _ in range(12):
            f = conv1_forward(img, w, gamma, beta, EPS32, MOM32, c["slope"], 0, 0, rm, rv)
            near = np.abs(f["z"]) < 4 * f["tau"]
            if not near.any():
                break
            # The channel's shift moves every z of the channel and no statistic: put the kink into the nearest gap between the
            # channel's sorted z that is wide enough.  (Moving pixels moves the batch statistics, hence every z of a channel with
            # few pixels; a sparse image gives most pixels of a channel the SAME z, nine background taps, which no pixel moves.)
            # Channels with too many pixels for such a gap move single pixels, whose effect on the statistics is small there.
            crowded = np.zeros(C, dtype=bool)
            for ch in np.nonzero(near.reshape(-1, C).any(0))[0]:
                zc = f["z"][..., ch].ravel()
                win = np.abs(zc) < 0.02
                need = 10 * f["tau"][..., ch].ravel()[win].max()
                edges = np.concatenate(([-0.02], np.sort(zc[win]), [0.02]))
                wide = np.nonzero(np.diff(edges) >= need)[0]
                if len(wide) == 0:
                    crowded[ch] = True
                    continue
                mid = 0.5 * (edges[wide] + edges[wide + 1])
                beta[ch] = f32(beta[ch] - mid[np.argmin(np.abs(mid))])
            n, h, ww = np.nonzero(near[..., crowded].any(-1))   # the centre tap (2h+1, 2w+1) belongs to this output pixel alone
            old = img[n, 2 * h + 1, 2 * ww + 1]
            img[n, 2 * h + 1, 2 * ww + 1] = round_half(np.where(old < 0.5, old + 0.25, old - 0.25), kind)
    return dict(img=img, w=w, dy=dy, gamma=gamma, beta=beta, running_mean=rm, running_var=rv)


ADAM_HYPER = dict(lr=float(np.float32(2e-4)), betas=(0.5, float(np.float32(0.999))), eps=float(np.float32(1e-7)))   # as the ABI's floats
ADAM_SCALE, ADAM_GROWTH, ADAM_BACKOFF, ADAM_INTERVAL = 1024.0, 2.0, 0.5, 3
ADAM_SIZES = (1, 7, 1023, 1025, 2048)


def adam_sets():
    """name -> list of parameter shapes; (8, 16, 4, 4) is held channels_last; `no_grad`: index of the parameter without gradient"""
    big = [(ADAM_SIZES[(3 * i + i // 5) % 5],) for i in range(130)]
    big[4] = (8, 16, 4, 4)
    assert big[4][0] * big[4][1] * 16 == 2048
    mid = [(ADAM_SIZES[(2 * i + 1) % 5],) for i in range(127)]
    return dict(global_table=dict(shapes=big, no_grad=9, channels_last=4),
                last_lds_table=dict(shapes=mid, no_grad=None, channels_last=None),
                tiny=dict(shapes=[(7,), (1,), (200,)], no_grad=None, channels_last=None))


def adam_flat_index(shapes, no_grad, flat):
    """(tensor, offset) of element `flat` of the concatenation of the tensors that have a gradient"""
    start = 0
    for i, s in enumerate(shapes):
        if i == no_grad:
            continue
        n = int(np.prod(s))
        if flat < start + n:
            return i, flat - start
        start += n
    raise IndexError(flat)


def adam_total(shapes, no_grad):
    return sum(int(np.prod(s)) for i, s in enumerate(shapes) if i != no_grad)


def make_adam(name, steps=12, seed=77):
    """parameters and per-step UNSCALED gradients (float32 values): magnitudes 1e-3 ... 10 across steps; in the global-table set four
    steps carry one non-finite value each: +inf at element 0 of tensor 0, NaN at the last element of the last tensor (the tail
    workgroup), -inf at flat index 1023 and at 1024 (the two sides of a workgroup boundary)."""
    s = adam_sets()[name]
    rng = np.random.default_rng(seed)
    shapes = s["shapes"]
    p = [f32(rng.standard_normal(sh) * 0.1) for sh in shapes]
    mags = (1e-3, 1.0, 10.0, 1e-2, 0.1, 3.0, 1e-3, 10.0, 0.3, 1.0, 1e-2, 5.0)
    grads, bad = [], {}
    for it in range(steps):
        gs = [None if i == s["no_grad"] else f32(rng.standard_normal(sh) * mags[it % len(mags)]) for i, sh in enumerate(shapes)]
        grads.append(gs)
    if name == "global_table":
        last = len(shapes) - 1
        bad = {2: (0, 0, np.inf), 5: (last, int(np.prod(shapes[last])) - 1, np.nan),
               8: adam_flat_index(shapes, s["no_grad"], 1023) + (-np.inf,), 10: adam_flat_index(shapes, s["no_grad"], 1024) + (-np.inf,)}
    elif steps > 4:
        bad = {4: (len(shapes) - 1, 0, np.nan)}
    for it, (ti, off, val) in bad.items():
        if it < steps:
            grads[it][ti].reshape(-1)[off] = val
    return dict(p=p, grads=grads, bad=bad, **s)
