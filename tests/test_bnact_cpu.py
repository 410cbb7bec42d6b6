"""The float64 twins, the bounds and the case table of bnact_common.py are fit to judge csrc/bnact.hip and csrc/optim.hip: the twins
agree with float64 PyTorch, every case keeps the kink caps, every case reaches the code path it is in the table for, and every
deliberate mutation of a twin leaves its bound on at least one case.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bnact_common as B

CU = 256                                                   # the MI355X; the GPU test asks the device
BN = B.bn_cases(CU)
C1 = B.conv1_cases(CU)
ids = lambda c: c["name"]


def eval_bn(c, mutation=None):
    d = B.make_bn(c)
    args = (d["gamma"], d["beta"], B.EPS32)
    f = B.bn_forward(d["x"], *args, B.MOM32, c["slope"], c["ph"], c["pw"], d["running_mean"], d["running_var"])
    b = B.bn_backward(d["x"], d["dy"], *args, c["slope"], c["ph"], c["pw"])
    L = B.chain_bn(c["N"] * c["H"] * c["W"], c["C"], CU)
    bd = B.bn_bounds(d["x"], *args, B.MOM32, c["slope"], f, b, L, c["kind"])
    if mutation is None:
        return d, f, b, bd
    fm = B.bn_forward(d["x"], *args, B.MOM32, c["slope"], c["ph"], c["pw"], d["running_mean"], d["running_var"], mutation)
    bm = B.bn_backward(d["x"], d["dy"], *args, c["slope"], c["ph"], c["pw"], mutation)
    return d, f, b, bd, fm, bm


def eval_conv1(c):
    d = B.make_conv1(c)
    args = (d["gamma"], d["beta"], B.EPS32)
    f = B.conv1_forward(d["img"], d["w"], *args, B.MOM32, c["slope"], c["ph"], c["pw"], d["running_mean"], d["running_var"])
    b = B.conv1_backward(d["img"], d["w"], d["dy"], *args, c["slope"], c["ph"], c["pw"])
    M = c["N"] * c["H"] * c["W"]
    bds = [B.conv1_bounds(d["img"], d["w"], *args, B.MOM32, c["slope"], f, b, B.chain_imgstats(M, CU),
                          B.chain_c1_bwd(c["N"], c["H"], c["W"], c["C"], CU, pk), c["kind"])
           for pk in ((False, True) if B.takes_packed(c["C"], c["W"]) else (False,))]
    return d, f, b, bds


def close(a, ref, rel=1e-12):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max()) <= rel * max(1.0, float(np.abs(ref).max()))


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


# ---- the twins against float64 PyTorch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in BN if not c.get("big") and c["N"] * c["H"] * c["W"] > 1], ids=ids)
def test_bn_twin_matches_float64_torch(c):
    d, f, b, _ = eval_bn(c)
    bn = torch.nn.BatchNorm2d(c["C"], eps=B.EPS32, momentum=B.MOM32).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(d["gamma"])); bn.bias.copy_(torch.from_numpy(d["beta"]))
        bn.running_mean.copy_(torch.from_numpy(d["running_mean"])); bn.running_var.copy_(torch.from_numpy(d["running_var"]))
    x = nchw(d["x"]).clone().requires_grad_(True)
    y = F.pad(F.leaky_relu(bn(x), c["slope"]), (0, c["pw"], 0, c["ph"]))
    dy = nchw(d["dy"])
    assert torch.isnan(dy).any() == bool(c.get("nan_pad") and (c["ph"] or c["pw"]))
    y.backward(dy)                                         # the pad's backward is a slice: it does not read the NaN either
    assert close(f["y"], nhwc(y)) and close(b["dx"], nhwc(x.grad))
    assert close(b["dgamma"], bn.weight.grad.numpy()) and close(b["dbeta"], bn.bias.grad.numpy())
    assert close(f["running_mean"], bn.running_mean.numpy()) and close(f["running_var"], bn.running_var.numpy())
    xs = d["x"].reshape(-1, c["C"])
    assert close(f["mean"], xs.mean(0)) and close(f["var"], xs.var(0)) and close(f["rstd"], 1 / np.sqrt(xs.var(0) + B.EPS32))
    assert np.isfinite(b["dx"]).all() and np.isfinite(b["dgamma"]).all() and np.isfinite(b["dbeta"]).all()


@pytest.mark.parametrize("c", [c for c in BN if c["N"] * c["H"] * c["W"] == 1], ids=ids)
def test_bn_twin_at_one_pixel(c):
    """BatchNorm2d refuses one value per channel; the kernel does not: var = 0, rstd = 1 / sqrt(eps), dx = 0, running_var moves by
    momentum * 0 (the unbiased factor is 1 at M = 1, as in k_bn_finalize)"""
    d, f, b, bd = eval_bn(c)
    assert np.all(f["var"] == 0) and close(f["rstd"], np.full(c["C"], 1 / np.sqrt(B.EPS32)))
    assert np.all(b["dx"] == 0) and close(f["running_var"], (1 - B.MOM32) * d["running_var"])
    assert np.array_equal(f["mean"], d["x"][0, 0, 0])


@pytest.mark.parametrize("c", [c for c in C1 if not c.get("big")], ids=ids)
def test_conv1_twin_matches_float64_torch(c):
    d, f, b, _ = eval_conv1(c)
    C = c["C"]
    conv = torch.nn.Conv2d(1, C, 3, stride=2, padding=0, bias=False).double()
    bn = torch.nn.BatchNorm2d(C, eps=B.EPS32, momentum=B.MOM32).double().train()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(d["w"].T.reshape(C, 1, 3, 3)))
        bn.weight.copy_(torch.from_numpy(d["gamma"])); bn.bias.copy_(torch.from_numpy(d["beta"]))
        bn.running_mean.copy_(torch.from_numpy(d["running_mean"])); bn.running_var.copy_(torch.from_numpy(d["running_var"]))
    y = F.pad(F.leaky_relu(bn(conv(torch.from_numpy(d["img"])[:, None])), c["slope"]), (0, c["pw"], 0, c["ph"]))
    y.backward(nchw(d["dy"]))
    assert close(f["y"], nhwc(y))
    assert close(b["dW"], conv.weight.grad.numpy().reshape(C, 9).T)
    assert close(b["dgamma"], bn.weight.grad.numpy()) and close(b["dbeta"], bn.bias.grad.numpy())
    assert close(f["running_mean"], bn.running_mean.numpy()) and close(f["running_var"], bn.running_var.numpy())


def _torch_adam_run(data, scaled):
    """torch.optim.Adam in float64 (+ GradScaler("cpu") when scaled) on the case's gradients: per step (p, scale, skipped)"""
    ps = [torch.from_numpy(a.copy()).requires_grad_(True) for a in data["p"]]
    opt = torch.optim.Adam(ps, lr=B.ADAM_HYPER["lr"], betas=B.ADAM_HYPER["betas"], eps=B.ADAM_HYPER["eps"])
    scaler = torch.amp.GradScaler("cpu", init_scale=B.ADAM_SCALE, growth_factor=B.ADAM_GROWTH, backoff_factor=B.ADAM_BACKOFF,
                                  growth_interval=B.ADAM_INTERVAL) if scaled else None
    out, scale = [], B.ADAM_SCALE
    for gs in data["grads"]:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.from_numpy(g * (scale if scaled else 1.0))
        before = [p.detach().clone() for p in ps]
        if scaled:
            scaler.scale(torch.zeros(()))
            scaler.step(opt)
            scaler.update()
            scale = float(scaler.get_scale())
        else:
            opt.step()
        out.append(([p.detach().numpy().copy() for p in ps], scale, all(torch.equal(a, p.detach()) for a, p in zip(before, ps))))
    return out, opt, ps


@pytest.mark.parametrize("name", sorted(B.adam_sets()))
def test_adam_twin_matches_float64_torch_adam_and_grad_scaler(name):
    data = B.make_adam(name)
    ref, opt, ps = _torch_adam_run(data, True)
    scale, traj = B.ADAM_SCALE, []
    state, p = None, data["p"]
    for gs in data["grads"]:                               # the gradients are scaled by the scale of their own step
        r = B.adam_steps(p, [[None if g is None else g * scale for g in gs]], scale=scale, growth=B.ADAM_GROWTH, backoff=B.ADAM_BACKOFF,
                         interval=B.ADAM_INTERVAL, state=state, **B.ADAM_HYPER)[0]
        traj.append(r)
        p, scale, state = r["p"], r["scale"], dict(m=r["m"], v=r["v"], t=r["t"], tracker=r["tracker"])
    for it, (r, (pt, st, unchanged)) in enumerate(zip(traj, ref)):
        assert r["scale"] == st and r["skipped"] == (it in data["bad"]), it
        assert r["skipped"] == unchanged or it == 0
        assert all(close(a, b_) for a, b_ in zip(r["p"], pt)), it
    assert sum(r["skipped"] for r in traj) == len(data["bad"]) and traj[-1]["t"] == len(traj) - len(data["bad"])
    for i, q in enumerate(ps):                             # the moments too
        if i != data["no_grad"]:
            assert close(traj[-1]["m"][i], opt.state[q]["exp_avg"].numpy()) and close(traj[-1]["v"][i], opt.state[q]["exp_avg_sq"].numpy())
    if data["no_grad"] is not None:
        assert np.array_equal(traj[-1]["p"][data["no_grad"]], data["p"][data["no_grad"]])
    # without a scale: plain Adam on the finite steps, nothing tested
    clean = dict(data, grads=[gs for it, gs in enumerate(data["grads"]) if it not in data["bad"]])
    ref2, _, _ = _torch_adam_run(clean, False)
    tr2 = B.adam_steps(clean["p"], clean["grads"], scale=None, growth=2.0, backoff=0.5, interval=3, **B.ADAM_HYPER)
    assert all(close(a, b_) for a, b_ in zip(tr2[-1]["p"], ref2[-1][0]))
    # and the same trajectory as the scaled run (the unscale by a power of two is exact)
    assert all(np.array_equal(a, b_) for a, b_ in zip(tr2[-1]["p"], traj[-1]["p"]))


# ---- the cases: caps on the kink, and the code path each is in the table for ------------------------------------------------------------
def _caps(f, bd, names):
    assert f["mask"].mean() <= 1e-3
    for k in names:
        assert np.all(bd["kink_" + k] <= 0.1 * bd["sum_" + k]), k


@pytest.mark.parametrize("c", BN, ids=ids)
def test_bn_case_keeps_the_kink_caps(c):
    d, f, b, bd = eval_bn(c)
    _caps(f, bd, ("dgamma", "dbeta"))
    if c["slope"] == 1.0:
        assert np.all(bd["kink_dgamma"] == 0) and np.all(bd["kink_dbeta"] == 0)
    if c.get("zero_channel"):                              # exact zeros of z, and not masked: tau is 0 there
        assert np.all(f["z"][..., 0] == 0) and not f["mask"][..., 0].any()
    for k in ("y", "dx", "mean", "rstd", "running_mean", "running_var", "dgamma", "dbeta"):
        assert np.isfinite(bd[k]).all() and np.all(bd[k] >= 0), k


@pytest.mark.parametrize("c", C1, ids=ids)
def test_conv1_case_keeps_the_kink_caps(c):
    d, f, b, bds = eval_conv1(c)
    for bd in bds:
        _caps(f, bd, ("dgamma", "dbeta", "dW"))
        for k in ("y", "mean", "rstd", "running_mean", "running_var", "dgamma", "dbeta", "dW"):
            assert np.isfinite(bd[k]).all() and np.all(bd[k] >= 0), k
    if c["sparse"] and d["img"].size > 1000:
        assert 0.9 < np.mean(d["img"][:, :-1, :-1] == -1.0) < 0.99
    assert np.all(d["img"][:, -1] == 0) and np.all(d["img"][:, :, -1] == 0)


def test_case_tables_reach_their_code_paths():
    cap = 8 * CU
    by = {c["name"]: c for c in BN}
    assert {c["C"] for c in BN if c["name"].startswith("c")} == set(B.ALL_C)
    for c in BN:
        M, PL = c["N"] * c["H"] * c["W"], 256 // (c["C"] // 8)
        if c.get("big"):                                   # some thread takes a second pixel, not every thread does
            assert cap * PL < M < 2 * cap * PL and B.stats_grid(M, c["C"], CU) == cap and B.chain_bn(M, c["C"], CU) == 2 + PL
            assert M * c["C"] * 2 <= 10.5e6
        elif c["name"].startswith("c"):
            assert M == 30 and (M < PL or M % PL or PL <= 2)
    for name, items in (("rows-c128-w15-h", 256), ("rows-c128-w16-h", 272), ("rows-c8-w255-b", 256), ("rows-c8-w300-b", 301)):
        c = by[name]
        assert (c["W"] + c["pw"]) * (c["C"] // 8) == items
    assert {(c["ph"], c["pw"]) for c in BN if c.get("nan_pad")} == {(0, 0), (1, 1), (0, 1), (1, 0)}
    assert all(c["abi"] for c in BN if c["ph"] != c["pw"])
    assert sum(1 for c in BN if c.get("ill")) == 7 and sum(1 for c in BN if c.get("outlier")) == 1
    for c in C1:
        N, H, W, C = c["N"], c["H"], c["W"], c["C"]
        four = C % 4 == 0 and 256 % (C // 4) == 0 and C // 4 <= 256
        assert four == (C != 2048)
        assert c.get("fwd_only", False) == (W > B.C1_BWD_MAX_W)
        if c["name"].startswith("c128-w8"):
            assert H != W and N * H > B.stats_grid(N * H * W, C, CU)          # the row stride of the general kernels
        if c["name"].startswith("c128-w72"):
            assert W > 8 * (256 // (C // 4)) and H != W                         # u0 > 0
        if c["name"].startswith("c1024-w9"):
            assert W > 8 * (256 // (C // 4))
        if c["name"].startswith("pk-"):
            assert B.takes_packed(C, W) and H != W or c["name"].startswith("pk-rows")
        if c["name"].startswith("pk-rows"):
            assert N * H > 8 * CU and N >= 100 and N * (H + 1) * (W + 1) * C * 2 <= 10.5e6     # more rows than workgroups can be resident
        if c["name"].startswith("imgstats2"):
            assert N * H * W > cap * 256
    assert {(c["ph"], c["pw"]) for c in C1} == {(1, 1), (0, 1), (1, 0)}
    sets = B.adam_sets()
    assert [len(s["shapes"]) - (s["no_grad"] is not None) for s in sets.values()] == [129, 127, 3]
    assert len(sets["global_table"]["shapes"]) == 130 and 129 > 127        # the table with the total entry: 130 > kMaxLds + 1 = 128
    for s in sets.values():
        assert B.adam_total(s["shapes"], s["no_grad"]) % 1024 != 0
    g = sets["global_table"]
    assert {int(np.prod(s)) for s in g["shapes"]} == set(B.ADAM_SIZES) and B.adam_total(sets["tiny"]["shapes"], None) < 256
    starts = np.cumsum([0] + [int(np.prod(s)) for i, s in enumerate(g["shapes"]) if i != g["no_grad"]])
    assert np.sum(starts % 1024 != 0) > 100                # tensor starts inside the 1024-element workgroups
    data = B.make_adam("global_table")
    vals = [data["grads"][it][ti].reshape(-1)[off] for it, (ti, off, _) in sorted(data["bad"].items())]
    assert np.isposinf(vals[0]) and np.isnan(vals[1]) and np.isneginf(vals[2]) and np.isneginf(vals[3]) and len(data["bad"]) == 4
    total = B.adam_total(g["shapes"], g["no_grad"])
    last = len(g["shapes"]) - 1
    assert data["bad"][5][:2] == (last, int(np.prod(g["shapes"][last])) - 1) and (total - 1) // 1024 == (total + 1023) // 1024 - 1


# ---- the bounds have teeth ------------------------------------------------------------------------------------------------------------
def _exceeds(value, ref, bound):
    return not np.all(np.abs(value - ref) <= bound)        # a NaN exceeds


def _bn_caught(mutation, pick):
    hit = []
    for c in BN:
        if c.get("big") or not pick(c):
            continue
        d, f, b, bd, fm, bm = eval_bn(c, mutation)
        H, W = c["H"], c["W"]
        out = {k: _exceeds(fm[k], f[k], bd[k]) for k in ("mean", "rstd", "running_mean", "running_var")}
        out["y"] = _exceeds(fm["y"][:, :H, :W], f["y"][:, :H, :W], bd["y"])
        keep = ~f["mask"]
        out["dx"] = _exceeds(bm["dx"][keep], b["dx"][keep], bd["dx"][keep])
        out.update({k: _exceeds(bm[k], b[k], bd[k]) for k in ("dgamma", "dbeta")})
        if any(out.values()):
            hit.append((c["name"], [k for k, v in out.items() if v]))
    return hit


@pytest.mark.parametrize("mutation,outputs", [("unbiased_var", {"rstd", "y"}), ("drop_last", {"mean", "rstd"}), ("roll_gamma", {"y", "dx"}),
                                              ("ge_zero", {"dbeta", "dx"}), ("c2_m1", {"dx"}), ("pad_from_dy", {"dx", "dbeta", "dgamma"})])
def test_bn_mutations_leave_the_bound(mutation, outputs):
    pick = {"ge_zero": lambda c: c.get("zero_channel") and c["slope"] != 1.0,
            "pad_from_dy": lambda c: c["ph"] == 1}.get(mutation, lambda c: c["N"] * c["H"] * c["W"] > 1)
    hit = _bn_caught(mutation, pick)
    assert hit, mutation
    assert any(outputs <= set(ks) for _, ks in hit), (mutation, hit[:3])
    if mutation == "ge_zero":                              # caught ONLY where z is exactly 0
        assert not _bn_caught(mutation, lambda c: not c.get("zero_channel") and c["slope"] != 1.0)


@pytest.mark.parametrize("mutation", ["bias_tm1", "v_scaled"])
def test_adam_mutations_leave_the_bound(mutation):
    """The mutated run continues from the unmutated state after two steps (t = 2), so the off-by-one bias correction uses t - 1 >= 2
    and stays finite: what leaves the bound is a finite error of one update, not a NaN from 1 - beta^0 = 0."""
    data = B.make_adam("tiny", steps=5)
    kw = dict(scale=B.ADAM_SCALE, growth=B.ADAM_GROWTH, backoff=B.ADAM_BACKOFF, interval=100, **B.ADAM_HYPER)
    grads = [[g * B.ADAM_SCALE for g in gs] for gs in data["grads"][:4]]
    head = B.adam_steps(data["p"], grads[:2], **kw)[-1]
    assert head["t"] == 2 and not head["skipped"]
    state = dict(m=head["m"], v=head["v"], t=head["t"], tracker=head["tracker"])
    ref = B.adam_steps(head["p"], grads[2:], state=state, **kw)
    mut = B.adam_steps(head["p"], grads[2:], state=state, mutation=mutation, **kw)
    assert all(np.isfinite(a).all() for m_ in mut for k in ("p", "m", "v") for a in m_[k])
    # one step: p against the bound of one update, m and v against their 2 ulps
    pb = B.adam_p_bound(ref[:1], head["p"], B.ADAM_HYPER["lr"], B.ADAM_HYPER["betas"])[0]
    caught_p = any(_exceeds(a, b_, bd) for a, b_, bd in zip(mut[0]["p"], ref[0]["p"], pb))
    mb, vb = zip(*[B.adam_mv_bound(m0, v0, g, B.ADAM_HYPER["betas"], m1, v1)
                   for m0, v0, g, m1, v1 in zip(head["m"], head["v"], data["grads"][2], ref[0]["m"], ref[0]["v"])])
    caught_v = any(_exceeds(a, b_, bd) for a, b_, bd in zip(mut[0]["v"], ref[0]["v"], vb))
    assert not any(_exceeds(a, b_, bd) for a, b_, bd in zip(mut[0]["m"], ref[0]["m"], mb))
    assert caught_p and caught_v == (mutation == "v_scaled")
    if mutation == "bias_tm1":                             # a finite, small error: a few per cent of one update of size <= lr
        worst = max(float(np.abs(a - b_).max()) for a, b_ in zip(mut[0]["p"], ref[0]["p"]))
        assert worst < 2 * B.ADAM_HYPER["lr"]


def test_half_rounding_and_ulps():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4096).astype(np.float32) * np.float32(7.0)
    assert np.array_equal(B.round_half(a, "bfloat16"), torch.from_numpy(a).bfloat16().double().numpy())
    assert np.array_equal(B.round_half(a, "float16"), torch.from_numpy(a).half().double().numpy())
    assert np.array_equal(B.to_bits(a, "bfloat16"), torch.from_numpy(a).bfloat16().view(torch.int16).numpy().view(np.uint16))
    assert B.ulp_h(1.0, "float16") == 2.0 ** -10 and B.ulp_h(0.999, "float16") == 2.0 ** -11 and B.ulp_h(0.0, "float16") == 2.0 ** -24
    assert B.ulp_h(3.0, "bfloat16") == 2.0 ** -6 and B.ulp32(1.0) == 2.0 ** -23 and B.ulp32(0.75) == 2.0 ** -24
