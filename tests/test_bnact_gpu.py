"""csrc/bnact.hip and csrc/optim.hip against the float64 twins of bnact_common.py, case by case, with the derived bounds of that
module (nothing here is tuned: a ratio error / bound above 1 fails).  Every test prints its worst ratio per quantity; the last test
prints the worst over the sweep -- the figures DESIGN.md 3.6 quotes under "Float64 sweep"."""
import importlib

import numpy as np
import pytest
import torch

import bnact_common as B

pytestmark = pytest.mark.gpu

CU = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
BN = B.bn_cases(CU)
C1 = B.conv1_cases(CU)
DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
WORST = {}                                                  # quantity -> (ratio, case)
ids = lambda c: c["name"]


def dev_half(a, kind):
    """NHWC float64 array of half-representable values (NaN allowed) -> contiguous (N, H, W, C) half tensor on the GPU"""
    return torch.from_numpy(B.to_bits(a, kind).view(np.int16)).cuda().view(DT[kind])


def dev_f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


class Judge:
    """collects error / bound per quantity for one case; `done` prints and asserts"""

    def __init__(self, case):
        self.case, self.worst = case, {}

    def add(self, name, got, ref, bound, keep=None):
        got, ref, bound = np.broadcast_arrays(np.asarray(got, dtype=np.float64), ref, bound)
        if keep is not None:
            got, ref, bound = got[keep], ref[keep], bound[keep]
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isfinite(got), ratio, np.inf)
        worst = float(ratio.max()) if ratio.size else 0.0
        if worst >= self.worst.get(name, (-1.0, 0.0))[0]:
            self.worst[name] = (worst, float(err.max()) if err.size else 0.0)
        if worst >= WORST.get(name, (-1.0, ""))[0]:
            WORST[name] = (worst, self.case)

    def done(self):
        print("\n%s: " % self.case + "  ".join("%s %.3g (err %.2e)" % ((k,) + v) for k, v in self.worst.items()))
        bad = [(k,) + v for k, v in self.worst.items() if not v[0] <= 1.0]
        assert not bad, (self.case, bad)


# ---- the C ABI, called the way BnLReluPad / Conv1BnLReluPad call it (pad_h != pad_w only exists here) ---------------------------------
def _ws(lib, _lib, C):
    return torch.empty((int(lib.rml_bn_workspace_floats(_lib.context(0), C)) + 2 * C,), dtype=torch.float32, device="cuda")


def abi_bn(c, d, backward=True):
    from radar_ml_amd import _lib
    lib = _lib.load()
    N, H, W, C, ph, pw = c["N"], c["H"], c["W"], c["C"], c["ph"], c["pw"]
    kind, dt = c["kind"], 1 if c["kind"] == "bfloat16" else 0
    x, gamma, beta = dev_half(d["x"], kind), dev_f32(d["gamma"]), dev_f32(d["beta"])
    rm, rv = dev_f32(d["running_mean"]), dev_f32(d["running_var"])
    y = torch.full((N, H + ph, W + pw, C), float("nan"), dtype=DT[kind], device="cuda")
    mean, rstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ws, hctx, st = _ws(lib, _lib, C), _lib.context(0), _lib.stream_ptr(0)
    p = _lib.ptr
    _lib.check(lib.rml_bn_lrelu_pad_forward(hctx, p(x), dt, N, H, W, C, ph, pw, p(gamma), p(beta), B.EPS, B.MOMENTUM, float(c["slope"]),
                                            p(rm), p(rv), p(mean), p(rstd), p(ws), p(y), st), "rml_bn_lrelu_pad_forward")
    out = dict(y=host(y), mean=host(mean), rstd=host(rstd), running_mean=host(rm), running_var=host(rv), y_t=y)
    if backward:
        dy = dev_half(d["dy"], kind)
        dx = torch.full((N, H, W, C), float("nan"), dtype=DT[kind], device="cuda")
        dgamma, dbeta = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        _lib.check(lib.rml_bn_lrelu_pad_backward(hctx, p(x), p(dy), dt, N, H, W, C, ph, pw, p(gamma), p(beta), p(mean), p(rstd),
                                                 float(c["slope"]), p(ws), p(dx), p(dgamma), p(dbeta), st), "rml_bn_lrelu_pad_backward")
        out.update(dx=host(dx), dgamma=host(dgamma), dbeta=host(dbeta))
    return out


def abi_conv1(c, d, backward=True):
    from radar_ml_amd import _lib
    lib = _lib.load()
    N, H, W, C, ph, pw = c["N"], c["H"], c["W"], c["C"], c["ph"], c["pw"]
    kind, dt = c["kind"], 1 if c["kind"] == "bfloat16" else 0
    img, wk, gamma, beta = dev_half(d["img"], kind), dev_f32(d["w"]), dev_f32(d["gamma"]), dev_f32(d["beta"])
    rm, rv = dev_f32(d["running_mean"]), dev_f32(d["running_var"])
    y = torch.full((N, H + ph, W + pw, C), float("nan"), dtype=DT[kind], device="cuda")
    mean, rstd, istat = torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(54, device="cuda")
    ws, hctx, st = _ws(lib, _lib, C), _lib.context(0), _lib.stream_ptr(0)
    p = _lib.ptr
    _lib.check(lib.rml_conv1_bn_lrelu_pad_forward(hctx, p(img), p(wk), dt, N, H, W, C, ph, pw, p(gamma), p(beta), B.EPS, B.MOMENTUM,
                                                  float(c["slope"]), p(rm), p(rv), p(mean), p(rstd), p(istat), p(ws), p(y), st),
               "rml_conv1_bn_lrelu_pad_forward")
    out = dict(y=host(y), mean=host(mean), rstd=host(rstd), running_mean=host(rm), running_var=host(rv), y_t=y)
    if backward:
        dy = dev_half(d["dy"], kind)
        dw, dgamma, dbeta = torch.empty((9, C), device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        _lib.check(lib.rml_conv1_bn_lrelu_pad_backward(hctx, p(img), p(wk), p(dy), dt, N, H, W, C, ph, pw, p(gamma), p(beta), p(mean),
                                                       p(rstd), p(istat), float(c["slope"]), p(ws), p(dw), p(dgamma), p(dbeta), st),
                   "rml_conv1_bn_lrelu_pad_backward")
        out.update(dW=host(dw), dgamma=host(dgamma), dbeta=host(dbeta))
    return out


def _bn_module(d, C):
    bn = torch.nn.BatchNorm2d(C, eps=B.EPS, momentum=B.MOMENTUM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(dev_f32(d["gamma"])); bn.bias.copy_(dev_f32(d["beta"]))
        bn.running_mean.copy_(dev_f32(d["running_mean"])); bn.running_var.copy_(dev_f32(d["running_var"]))
    return bn


def _judge_forward(j, got, f, bd, H, W):
    j.add("y", got["y"][:, :H, :W], f["y"][:, :H, :W], bd["y"])
    assert np.all(got["y"][:, H:] == 0) and np.all(got["y"][:, :, W:] == 0)        # pad row and column: exactly 0
    for k in ("mean", "rstd", "running_mean", "running_var"):
        if k in got:
            j.add(k, got[k], f[k], bd[k])


# ---- BatchNorm + activation + pad ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", BN, ids=ids)
def test_bn_lrelu_pad_against_float64(rml, c):
    nc = importlib.import_module("radar_ml_amd.nn_common")
    d = B.make_bn(c)
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    args = (d["gamma"], d["beta"], B.EPS32)
    f = B.bn_forward(d["x"], *args, B.MOM32, c["slope"], c["ph"], c["pw"], d["running_mean"], d["running_var"])
    b = B.bn_backward(d["x"], d["dy"], *args, c["slope"], c["ph"], c["pw"])
    bd = B.bn_bounds(d["x"], *args, B.MOM32, c["slope"], f, b, B.chain_bn(N * H * W, C, CU), c["kind"])
    j = Judge(c["name"])
    got = abi_bn(c, d, backward=c["abi"])                   # save_mean and save_rstd are the entry point's alone
    if not c["abi"]:
        bn = _bn_module(d, C)
        x = dev_half(d["x"], c["kind"]).permute(0, 3, 1, 2).requires_grad_(True)
        y = nc.bn_lrelu_pad(x, bn, c["slope"], c["ph"])
        assert y.is_contiguous(memory_format=torch.channels_last) and int(bn.num_batches_tracked) == 1
        assert torch.equal(y.detach().permute(0, 2, 3, 1), got["y_t"])            # fixed summation order: the same bits again
        y.backward(dev_half(d["dy"], c["kind"]).permute(0, 3, 1, 2))
        got.update(dx=host(x.grad.permute(0, 2, 3, 1)), dgamma=host(bn.weight.grad), dbeta=host(bn.bias.grad))
        assert np.array_equal(host(bn.running_mean), got["running_mean"]) and np.array_equal(host(bn.running_var), got["running_var"])
    _judge_forward(j, got, f, bd, H, W)
    j.add("dx", got["dx"], b["dx"], bd["dx"], keep=~f["mask"])
    j.add("dgamma", got["dgamma"], b["dgamma"], bd["dgamma"])
    j.add("dbeta", got["dbeta"], b["dbeta"], bd["dbeta"])
    if N * H * W == 1:                                      # one value per channel: var = 0 and the gradient vanishes exactly
        assert np.all(got["dx"] == 0) and np.array_equal(got["mean"], d["x"][0, 0, 0])
        assert np.array_equal(got["rstd"], np.full(C, np.float32(1.0 / np.sqrt(np.float64(B.EPS32))), dtype=np.float64))
    j.done()


# ---- the first layer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C1, ids=ids)
def test_conv1_bn_lrelu_pad_against_float64(rml, rml_opt, c):
    nc = importlib.import_module("radar_ml_amd.nn_common")
    d = B.make_conv1(c)
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    M = N * H * W
    args = (d["gamma"], d["beta"], B.EPS32)
    f = B.conv1_forward(d["img"], d["w"], *args, B.MOM32, c["slope"], c["ph"], c["pw"], d["running_mean"], d["running_var"])
    b = B.conv1_backward(d["img"], d["w"], d["dy"], *args, c["slope"], c["ph"], c["pw"])
    ys = []
    for pk in ((1, 0) if B.takes_packed(C, W) else (1,)):   # c1_pk = 1 is the default; other shapes take the general kernels anyway
        rml_opt("c1_pk", pk)
        packed = bool(pk) and B.takes_packed(C, W)
        bd = B.conv1_bounds(d["img"], d["w"], *args, B.MOM32, c["slope"], f, b, B.chain_imgstats(M, CU),
                            B.chain_c1_bwd(N, H, W, C, CU, packed), c["kind"])
        j = Judge(c["name"] + ("/packed" if packed else "/general"))
        got = abi_conv1(c, d, backward=c["abi"])
        if not c["abi"]:
            bn = _bn_module(d, C)
            conv = torch.nn.Conv2d(1, C, 3, stride=2, padding=0).cuda()
            with torch.no_grad():
                conv.weight.copy_(dev_f32(d["w"].T.reshape(C, 1, 3, 3))); conv.bias.zero_()
            with torch.set_grad_enabled(not c.get("fwd_only")):
                y = nc.conv1_bn_lrelu_pad(dev_f32(d["img"])[:, None], conv, bn, c["slope"], c["ph"], DT[c["kind"]])
            assert torch.equal(y.detach().permute(0, 2, 3, 1), got["y_t"])
            assert np.array_equal(host(bn.running_mean), got["running_mean"]) and np.array_equal(host(bn.running_var), got["running_var"])
            if not c.get("fwd_only"):
                y.backward(dev_half(d["dy"], c["kind"]).permute(0, 3, 1, 2))
                assert float(conv.bias.grad.abs().max()) == 0.0
                got.update(dW=host(conv.weight.grad.reshape(C, 9).t()), dgamma=host(bn.weight.grad), dbeta=host(bn.bias.grad))
        _judge_forward(j, got, f, bd, H, W)
        for k in ("dW", "dgamma", "dbeta"):
            if k in got:
                j.add("c1_" + k, got[k], b[k], bd[k])
        ys.append(got["y_t"])
        j.done()
    if len(ys) == 2:                                        # packed and general forward: the same products in the same order
        assert torch.equal(ys[0], ys[1])


def test_conv1_backward_refuses_rows_it_cannot_stage(rml):
    """k_c1_bwd1 keeps the three image rows of an output row in 2048 floats of LDS: rows of more than 340 pixels are an error (the
    longest accepted row is judged against the twin with the other cases: c8-w340)"""
    from radar_ml_amd import _lib
    nc = importlib.import_module("radar_ml_amd.nn_common")
    assert any(c["W"] == B.C1_BWD_MAX_W and not c.get("fwd_only") for c in C1)
    W = B.C1_BWD_MAX_W + 1
    conv = torch.nn.Conv2d(1, 8, 3, stride=2, padding=0).cuda()
    bn = torch.nn.BatchNorm2d(8, eps=B.EPS, momentum=B.MOMENTUM).cuda().train()
    torch.manual_seed(4)
    y = nc.conv1_bn_lrelu_pad(torch.rand((1, 1, 3, 2 * W + 1), device="cuda"), conv, bn, 0.2, 1, torch.float16)
    with pytest.raises(_lib.RadarMLError, match="rows of %d pixels" % W):
        y.backward(torch.ones_like(y))
    assert conv.weight.grad is None


# ---- Adam with the loss-scale rule ---------------------------------------------------------------------------------------------------
def _adam_tensors(data, arrays):
    out = []
    for i, a in enumerate(arrays):
        t = None if a is None else dev_f32(a)
        if t is not None and i == data["channels_last"]:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t)
    return out


@pytest.mark.parametrize("name", sorted(B.adam_sets()))
def test_device_adam_against_float64(rml, name):
    nc = importlib.import_module("radar_ml_amd.nn_common")
    data = B.make_adam(name)
    hy, betas = B.ADAM_HYPER, B.ADAM_HYPER["betas"]
    mk = lambda: [t.requires_grad_(True) for t in _adam_tensors(data, data["p"])]
    params, plain = mk(), mk()
    if data["channels_last"] is not None:
        assert params[data["channels_last"]].stride() != params[data["channels_last"]].contiguous().stride()
    scale = torch.full((1,), B.ADAM_SCALE, device="cuda")
    opt = nc.DeviceAdam(params, 2e-4, (0.5, 0.999), 1e-7, scale=scale, growth=B.ADAM_GROWTH, backoff=B.ADAM_BACKOFF,
                        growth_interval=B.ADAM_INTERVAL)
    ref = nc.DeviceAdam(plain, 2e-4, (0.5, 0.999), 1e-7)    # scale=None on the unscaled gradients: the same bits
    # the whole run of the twin (for p), with every step's gradients scaled by the scale of that step
    traj, s, st, p = [], B.ADAM_SCALE, None, data["p"]
    for gs in data["grads"]:
        r = B.adam_steps(p, [[None if g is None else g * s for g in gs]], scale=s, growth=B.ADAM_GROWTH, backoff=B.ADAM_BACKOFF,
                         interval=B.ADAM_INTERVAL, state=st, **hy)[0]
        traj.append(r)
        p, s, st = r["p"], r["scale"], dict(m=r["m"], v=r["v"], t=r["t"], tracker=r["tracker"])
    pbound = B.adam_p_bound(traj, data["p"], hy["lr"], betas)
    j = Judge("adam/" + name)
    live = [i for i in range(len(params)) if i != data["no_grad"]]
    for it, gs in enumerate(data["grads"]):
        s_now = float(scale)
        assert s_now == (traj[it - 1]["scale"] if it else B.ADAM_SCALE)
        for t, g in zip(params, _adam_tensors(data, [None if g is None else g * s_now for g in gs])):
            t.grad = g
        before = dict(p=[t.detach().clone(memory_format=torch.preserve_format) for t in params],
                      m=[t.clone(memory_format=torch.preserve_format) for t in opt.exp_avg],
                      v=[t.clone(memory_format=torch.preserve_format) for t in opt.exp_avg_sq],
                      t=float(opt.step_count), tracker=int(opt.state[1]))
        opt.step()
        r = traj[it]
        assert r["skipped"] == (it in data["bad"])
        assert float(scale) == r["scale"] and int(opt.state[1]) == r["tracker"] and float(opt.step_count) == r["t"], it
        if r["skipped"]:                                    # bit-unchanged, the step count too, the scale backed off
            for k, now in (("p", params), ("m", opt.exp_avg), ("v", opt.exp_avg_sq)):
                assert all(torch.equal(a, b_.detach()) for a, b_ in zip(before[k], now)), (it, k)
            assert float(opt.step_count) == before["t"] and float(scale) == s_now * B.ADAM_BACKOFF
            continue
        # one step of the twin from the kernel's own previous state: m and v within 2 float32 ulps
        one = B.adam_steps([host(t) for t in before["p"]], [[None if g is None else g * s_now for g in gs]], scale=s_now,
                           growth=B.ADAM_GROWTH, backoff=B.ADAM_BACKOFF, interval=B.ADAM_INTERVAL,
                           state=dict(m=[host(t) for t in before["m"]], v=[host(t) for t in before["v"]], t=before["t"],
                                      tracker=before["tracker"]), **hy)[0]
        for i in live:
            mb, vb = B.adam_mv_bound(host(before["m"][i]), host(before["v"][i]), gs[i], betas, one["m"][i], one["v"][i])
            j.add("adam_m", host(opt.exp_avg[i]), one["m"][i], mb)
            j.add("adam_v", host(opt.exp_avg_sq[i]), one["v"][i], vb)
            j.add("adam_p", host(params[i]), r["p"][i], pbound[it][i])
        if data["no_grad"] is not None:
            assert torch.equal(params[data["no_grad"]].detach(), before["p"][data["no_grad"]])
        # the unscale by a power of two is exact: the unscaled run gives the same bits
        for t, g in zip(plain, _adam_tensors(data, gs)):
            t.grad = g
        ref.step()
        for a, b_ in ((params, plain), (opt.exp_avg, ref.exp_avg), (opt.exp_avg_sq, ref.exp_avg_sq)):
            assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b_)), it
    assert float(opt.step_count) == len(data["grads"]) - len(data["bad"]) == float(ref.step_count)
    j.done()


def test_zz_worst_ratios_of_the_sweep():
    """prints error / bound, the worst over every case above that ran in this session"""
    for k in sorted(WORST):
        print("float64 sweep: %-14s worst error / bound = %.3g  (%s)" % (k, WORST[k][0], WORST[k][1]))
    assert all(v[0] <= 1.0 for v in WORST.values())
