"""csrc/conv_train.hip against the float64 twins of conv_train_common.py with the derived bounds of that module (nothing here is tuned:
a ratio error / bound above 1 fails), and the `convolutions="hip"` discriminator step built on it.  Every test prints its worst ratio
per quantity -- the figures DESIGN.md 3.6e quotes.

Measured on an MI355X: worst error / bound float16 0.43 / 0.92 / 0.97 (forward / data gradient / weight gradient),
bfloat16 0.86 / 0.99 / 0.996; gradients of the hip step against the float32 CPU step
(test_hip_step_gradients_against_the_float32_cpu_step): ratio of the hip error to the library error per tensor 0.85 on average, 1.89 at
worst, over 74 tensors."""
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_train_common as T
from bnact_common import to_bits

pytestmark = pytest.mark.gpu

CASES = T.cases()
DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
FWD, DGRAD, WGRAD = 0, 1, 2
RML_ERR_UNSUPPORTED = -2
ids = lambda c: c["name"]
_DATA = {}


def data(c):
    """the case's arrays and float64 references, computed once and never written to"""
    if c["name"] not in _DATA:
        d = T.make(c)
        d["Z"], d["dX"], d["dW"] = T.forward(d["X"], d["W"]), T.dgrad(d["dZ"], d["W"]), T.wgrad(d["X"], d["dZ"])
        for v in d.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
        _DATA[c["name"]] = d
    return _DATA[c["name"]]


def dev_half(a, kind):
    return torch.from_numpy(to_bits(a, kind).view(np.int16)).cuda().view(DT[kind])


def host(t):
    return t.detach().double().cpu().numpy()


def nan_like(shape, kind):
    return torch.full(shape, float("nan"), dtype=DT[kind], device="cuda")


def abi(which, c, a, b, out, cin=None, cout=None, hp=None, wp=None):
    """one pass through the C ABI with a NaN-filled workspace; returns the status"""
    from radar_ml_amd import _lib
    lib = _lib.load()
    cin, cout = cin or c["cin"], cout or c["cout"]
    hp, wp = hp or 2 * c["Ho"] + 1, wp or 2 * c["Wo"] + 1
    hctx = _lib.context(0)
    nbytes = int(lib.rml_conv3s2_workspace_bytes(hctx, c["N"], hp, wp, cin, cout, which))
    ws = torch.full((max(nbytes, 16) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    fn = (lib.rml_conv3s2_forward, lib.rml_conv3s2_dgrad, lib.rml_conv3s2_wgrad)[which]
    return fn(hctx, _lib.ptr(a), _lib.ptr(b), 1 if c["kind"] == "bfloat16" else 0, c["N"], hp, wp, cin, cout, _lib.ptr(out), _lib.ptr(ws),
              nbytes, _lib.stream_ptr(0))


def three_passes(c, d):
    kind = c["kind"]
    x, w, dz = dev_half(d["X"], kind), dev_half(d["W"], kind), dev_half(d["dZ"], kind)
    z, dx, dw = nan_like(d["Z"][0].shape, kind), nan_like(d["X"].shape, kind), nan_like(d["W"].shape, kind)
    assert abi(FWD, c, x, w, z) == 0 and abi(DGRAD, c, dz, w, dx) == 0 and abi(WGRAD, c, x, dz, dw) == 0
    torch.cuda.synchronize()
    return z, dx, dw


def judge(c, got, d, chain):
    """error / bound of the three outputs; prints the worst ratios and asserts"""
    n = T.chains(c, chain)
    worst = {}
    for name, key, g in (("forward", "Z", got[0]), ("dgrad", "dX", got[1]), ("wgrad", "dW", got[2])):
        if g is None:
            continue
        ref, asum = d[key]
        g = host(g)
        assert g.shape == ref.shape, name
        b = T.bound(ref, asum, n[name], c["kind"])
        ratio = np.where(np.isfinite(g), np.abs(g - ref) / b, np.inf)
        worst[name] = (float(ratio.max()), float(np.abs(g - ref).max()))
    print("\n%s: " % c["name"] + "  ".join("%s %.3g (err %.2e)" % ((k,) + v) for k, v in worst.items()))
    bad = [(k,) + v for k, v in worst.items() if not v[0] <= 1.0]
    assert not bad, (c["name"], bad)
    return worst


def _chain():
    return importlib.import_module("radar_ml_amd.nn_common").conv3s2_wgrad_chain


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_three_passes_against_float64(rml, c):
    d = data(c)
    got = three_passes(c, d)
    judge(c, got, d, _chain())
    again = three_passes(c, d)                              # the same bits on a second call
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("c", [c for c in CASES if c["path"] in ("tail", "mini") and not c["sparse"]], ids=ids)
def test_forward_bits_of_a_sample_do_not_depend_on_the_batch(rml, c):
    d = data(c)
    kind = c["kind"]
    x, w = dev_half(d["X"], kind), dev_half(d["W"], kind)
    z = nan_like(d["Z"][0].shape, kind)
    assert abi(FWD, c, x, w, z) == 0
    one = dict(c, N=1)
    for pos in (0, c["N"] - 1):
        # the sample alone, and moved to the other end of the batch
        z1 = nan_like((1,) + d["Z"][0].shape[1:], kind)
        assert abi(FWD, one, x[pos:pos + 1].contiguous(), w, z1) == 0
        assert torch.equal(z1.view(torch.int16), z[pos:pos + 1].view(torch.int16)), pos
        other = c["N"] - 1 - pos
        perm = list(range(c["N"]))
        perm[pos], perm[other] = perm[other], perm[pos]
        zp = nan_like(d["Z"][0].shape, kind)
        assert abi(FWD, c, x[perm].contiguous(), w, zp) == 0
        assert torch.equal(zp[other].view(torch.int16), z[pos].view(torch.int16)), pos


def test_unsupported_shapes_are_refused_before_any_launch(rml):
    from radar_ml_amd import _lib
    lib = _lib.load()
    assert lib.rml_conv3s2_supported(128, 64, 9, 9) == 1 and lib.rml_conv3s2_supported(64, 32, 5, 131) == 1
    for cin, cout, hp, wp in ((128, 32, 9, 9), (64, 64, 9, 9), (96, 64, 9, 9), (128, 64, 8, 9), (128, 64, 9, 10), (64, 32, 1, 9)):
        assert lib.rml_conv3s2_supported(cin, cout, hp, wp) == 0
        assert lib.rml_conv3s2_workspace_bytes(_lib.context(0), 2, hp, wp, cin, cout, FWD) == 0
        c = dict(kind="float16", N=2, Ho=(hp - 1) // 2, Wo=(wp - 1) // 2, cin=cin, cout=cout)
        a = torch.zeros((2 * hp * wp * 128,), dtype=torch.float16, device="cuda")
        b = torch.zeros((2 * hp * wp * 128,), dtype=torch.float16, device="cuda")
        for which in (FWD, DGRAD, WGRAD):
            out = nan_like((2 * hp * wp * 128,), "float16")
            assert abi(which, c, a, b, out, hp=hp, wp=wp) == RML_ERR_UNSUPPORTED, (cin, cout, hp, wp, which)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all())
            assert lib.rml_last_error()


@pytest.mark.parametrize("c", [c for c in CASES if c["path"] in ("one", "tail", "mini", "split")], ids=ids)
def test_autograd_wrapper_against_float32_conv2d(rml, c):
    nc = importlib.import_module("radar_ml_amd.nn_common")
    d = data(c)
    kind = c["kind"]
    x = dev_half(d["X"], kind).permute(0, 3, 1, 2).requires_grad_(True)           # channels_last views of the NHWC arrays
    w = dev_half(d["W"], kind).permute(0, 3, 1, 2).requires_grad_(True)
    dz = dev_half(d["dZ"], kind).permute(0, 3, 1, 2)
    assert nc.conv3s2_supported(x, w)
    z = nc.conv3s2(x, w)
    assert z.dtype == DT[kind] and z.is_contiguous(memory_format=torch.channels_last)
    gx, gw = torch.autograd.grad(z, (x, w), dz)
    # float32 F.conv2d and its autograd on the same values (on the host: no library in the reference)
    x32, w32 = x.detach().float().cpu().requires_grad_(True), w.detach().float().cpu().requires_grad_(True)
    z32 = F.conv2d(x32, w32, None, stride=2)
    gx32, gw32 = torch.autograd.grad(z32, (x32, w32), dz.float().cpu())
    ref = dict(Z=(host(z32).transpose(0, 2, 3, 1), d["Z"][1]), dX=(host(gx32).transpose(0, 2, 3, 1), d["dX"][1]),
               dW=(host(gw32).transpose(0, 2, 3, 1), d["dW"][1]))
    got = tuple(t.detach().permute(0, 2, 3, 1) for t in (z, gx, gw))
    judge(c, got, ref, _chain())
    judge(c, got, d, _chain())


def test_backward_computes_only_what_is_asked(rml, monkeypatch):
    nc = importlib.import_module("radar_ml_amd.nn_common")
    from radar_ml_amd import _lib
    lib = _lib.load()
    calls = []
    for name in ("rml_conv3s2_dgrad", "rml_conv3s2_wgrad"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append(name), real(*a))[1])(real, name), raising=False)
    c = next(c for c in CASES if c["path"] == "mini" and c["kind"] == "float16" and c["cin"] == 64 and not c["sparse"])
    d = data(c)
    dz = dev_half(d["dZ"], "float16").permute(0, 3, 1, 2)
    both = None
    for need_x, need_w in ((True, True), (True, False), (False, True)):
        x = dev_half(d["X"], "float16").permute(0, 3, 1, 2).requires_grad_(need_x)
        w = dev_half(d["W"], "float16").permute(0, 3, 1, 2).requires_grad_(need_w)
        z = nc.conv3s2(x, w)
        del calls[:]
        z.backward(dz)
        # the passes that ran are the gradients that were asked for: the other slot of backward's result is None
        assert sorted(calls) == [n for n, need in (("rml_conv3s2_dgrad", need_x), ("rml_conv3s2_wgrad", need_w)) if need]
        assert (x.grad is not None) == need_x and (w.grad is not None) == need_w
        if both is None:
            both = (x.grad.clone(), w.grad.clone())
        if need_x:
            assert torch.equal(x.grad, both[0])
        if need_w:
            assert torch.equal(w.grad, both[1])
    x = dev_half(d["X"], "float16").permute(0, 3, 1, 2)
    w = dev_half(d["W"], "float16").permute(0, 3, 1, 2)
    assert nc.conv3s2(x, w).grad_fn is None


# ---- the trainer: 16 x 16 planes, batch 8 -- the smallest size Discriminator._branch fuses -----------------------------------------------
def _base(seed=5):
    sgan = importlib.import_module("radar_ml_amd.sgan")
    torch.manual_seed(seed)
    return sgan, sgan.Discriminator(((16, 16, 1),) * 3, 3).to("cuda").to(memory_format=torch.channels_last)


def _batches(steps, seed=6):
    rng = np.random.default_rng(seed)
    return [([rng.uniform(-1, 1, (8, 16, 16, 1)).astype(np.float32) for _ in range(3)], rng.integers(0, 3, 8),
             [rng.uniform(-1, 1, (8, 16, 16, 1)).astype(np.float32) for _ in range(3)]) for _ in range(steps)]


def test_hip_step_is_reproducible_bit_for_bit(rml):
    sgan, base = _base()
    batches = _batches(3)
    runs = []
    for _ in range(2):
        net = copy.deepcopy(base)
        torch.manual_seed(11)                                # dropout masks
        tr = sgan.DiscriminatorTrainer(net, amp_dtype="float16", ddp=False, convolutions="hip")
        assert net.conv_impl == "hip"
        losses = []
        for x, y, xf in batches:                            # c + d + d on fakes
            losses.append(tr.train_on_batch_c(x, y)[0])
            losses.append(tr.train_on_batch_d(x, np.full((8, 1), 0.9)))
            losses.append(tr.train_on_batch_d(xf, np.zeros((8, 1))))
        state = {k: v.clone() for k, v in net.state_dict().items()}
        adam = [t.clone() for o in tr._dev_adam.values() for t in o.exp_avg + o.exp_avg_sq] if tr._dev_adam else \
               [v.clone() for o in (tr.opt_c, tr.opt_d) for s in o.state.values() for v in s.values() if torch.is_tensor(v)]
        runs.append((losses, state, adam))
    assert runs[0][0] == runs[1][0]
    assert all(np.isfinite(runs[0][0]))
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert len(runs[0][2]) == len(runs[1][2]) > 0
    for a, b in zip(runs[0][2], runs[1][2]):
        assert torch.equal(a, b)
    # the weights of layers 2 and 3 did move
    for k, v in base.state_dict().items():
        if k.endswith("3.conv.weight") or k.endswith("6.conv.weight"):
            assert not torch.equal(v, runs[0][1][k]), k


def test_hip_trainer_graph_matches_eager(rml):
    """what test_sgan_trainer_hip_graph_matches_eager asserts for the library, with convolutions="hip" """
    sgan, base = _base()
    base.drop.p = 0.0
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    trs = [sgan.DiscriminatorTrainer(nets[0], amp_dtype="float16", ddp=False, use_graph=False, convolutions="hip"),
           sgan.DiscriminatorTrainer(nets[1], amp_dtype="float16", ddp=False, use_graph=True, convolutions="hip")]
    hist = [[], []]
    for x, y, _ in _batches(7):
        for i, tr in enumerate(trs):
            lc, _ = tr.train_on_batch_c(x, y)
            ld = tr.train_on_batch_d(x, np.full((8, 1), 0.9))
            hist[i].append((lc, ld))
    assert "graph" in trs[1]._graphs["c"] and "graph" in trs[1]._graphs["d"]
    a, b = np.array(hist[0]), np.array(hist[1])
    print("\nhip graph vs eager: worst loss difference %.3g" % np.abs(a - b).max())
    assert np.abs(a - b).max() < 2e-2, (a, b)
    sd0, sd1 = nets[0].state_dict(), nets[1].state_dict()
    for k in sd0:
        if k.endswith("num_batches_tracked"):
            assert int(sd0[k]) == 14 and int(sd1[k]) == 14, k
        elif "running_" in k:
            assert (sd0[k] - sd1[k]).abs().max() <= 6e-3 * (1 + sd0[k].abs().max()), k
        elif k.endswith(".conv.bias"):
            assert torch.equal(sd0[k], base.state_dict()[k]) and torch.equal(sd1[k], base.state_dict()[k]), k


def _kinks_into_gaps(model, x):
    """A condition on the CASE, from the float32 CPU forward alone (the way bnact_common.make_conv1 conditions its cases): a LeakyReLU
    input that lies within half-precision round-off of zero takes either slope depending on the summation order in front of it, and at
    batch 8 ONE such element of the dense tail moves every gradient behind it by more than all other round-off together -- in either
    path, at random.  So every BatchNorm's beta is shifted, channel by channel and layer by layer in forward order, to put the kink in
    the middle of the widest gap between the channel's sorted pre-activations (a shift moves every z of the channel and no
    statistic).  Returns the smallest |z| per layer afterwards."""
    probe = copy.deepcopy(model).float().cpu()
    probe.train()
    bns = [[list(br)[i] for br in probe.branches] for i in (1, 4, 7)] + [[probe.bn1], [probe.bn2]]
    own = [[list(br)[i] for br in model.branches] for i in (1, 4, 7)] + [[model.bn1], [model.bn2]]
    margins = []
    for layer, mine in zip(bns, own):
        seen = {}
        hooks = [bn.register_forward_hook(lambda m, i, o: seen.__setitem__(id(m), o.detach())) for bn in layer]
        with torch.no_grad():
            probe(*x)
        for h in hooks:
            h.remove()
        worst = float("inf")
        for bn, target in zip(layer, mine):
            z = seen[id(bn)].double()
            z = z.transpose(0, 1).reshape(z.shape[1], -1)                 # (C, values)
            srt, _ = torch.sort(z, dim=1)
            gaps = srt[:, 1:] - srt[:, :-1]
            i = gaps.argmax(dim=1, keepdim=True)
            mid = 0.5 * (srt.gather(1, i) + srt.gather(1, i + 1)).squeeze(1)
            worst = min(worst, float((z - mid[:, None]).abs().min()))
            with torch.no_grad():
                bn.bias -= mid.to(bn.bias.dtype)
                target.bias -= mid.to(target.bias.dtype).to(target.bias.device)
        margins.append(round(worst, 5))
    return margins


def test_hip_step_gradients_against_the_float32_cpu_step(rml):
    """Per-parameter gradients of one c and one d update, float16 autocast on the GPU, against the plain float32 step on the CPU with the
    same weights and inputs: the error of every tensor with "hip" is at most twice its error with "library" in this same test (this
    project's margin for two half-precision paths that differ only in summation order).  Both errors are printed.  The model's
    BatchNorm shifts are conditioned first (_kinks_into_gaps)."""
    sgan, base = _base()
    base.drop.p = 0.0
    base.train()
    g = torch.Generator().manual_seed(6)
    x = [(torch.rand((8, 1, 16, 16), generator=g) * 2 - 1) for _ in range(3)]
    y = torch.randint(0, 3, (8,), generator=g)
    yr = torch.full((8,), 0.9)
    print("\nsmallest |pre-activation| of the float32 reference per layer:", _kinks_into_gaps(base, x))
    ref = copy.deepcopy(base).float().cpu()

    def grads(model, dev, head, autocast):
        model.zero_grad(set_to_none=True)
        xs = [t.to(dev).contiguous(memory_format=torch.channels_last) for t in x]
        if autocast:
            with torch.autocast("cuda", dtype=torch.float16):
                logits = model(*xs)
        else:
            logits = model(*xs)
        loss = sgan.c_loss(logits, y.to(dev)) if head == "c" else sgan.d_loss(logits, yr.to(dev))
        (loss * 256.0).backward()                           # a fixed loss scale keeps the float16 gradients out of the subnormals
        return {k: p.grad.detach().double().cpu() / 256.0 for k, p in model.named_parameters() if p.grad is not None}

    bad, lines = [], []
    for head in ("c", "d"):
        g32 = grads(copy.deepcopy(ref), "cpu", head, False)
        errs = {}
        for impl in ("library", "hip"):
            net = copy.deepcopy(base)
            net.conv_impl = impl
            g16 = grads(net, "cuda", head, True)
            errs[impl] = {k: float((g16[k] - g32[k].double()).norm()) for k in g16 if not k.endswith(".conv.bias")}
        assert set(errs["hip"]) == set(errs["library"]) and len(errs["hip"]) >= 30
        for k in sorted(errs["hip"]):
            eh, el = errs["hip"][k], errs["library"][k]
            lines.append("%s %-32s hip %.3e library %.3e ratio %.2f" % (head, k, eh, el, eh / el if el else float("inf") if eh else 0.0))
            if not eh <= 2.0 * el:
                bad.append((head, k, eh, el))
    print("\n" + "\n".join(lines))
    assert not bad, bad
