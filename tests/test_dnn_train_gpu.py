"""The CNN training step on the GPU (csrc/dnn_train.hip) against its float64 CPU twin (tests/dnn_train_common.py).

Bound: per parameter tensor e = max|g - g64| / max|g64| <= 8 x E32, E32 the largest e the float32 CPU twin shows over the cases
(computed here, at run time).  The factor 8 covers another summation order (per-workgroup partial sums against PyTorch's blocking);
an indexing or padding mistake is >= 1e-3 on these cases.  The loss has the same bound, the correct count is equal.  Trajectories
(20 Adam steps; fit end to end): 8 x the float32 twin's own deviation after the same steps, taken on the WEIGHTS (max|dw| / max|w| over the
tensors); a fit's history is held to that same trajectory bound, relative to the largest float64 value of the key -- not to the float32
twin's own history error, which for a float32 sum of a few dozen losses can fall below float32 resolution by chance (seen: 7e-9 on a
loss of 3.4) and depends on the host's summation blocking.  One sample's worth of accuracy is far above any such bound."""


def history_within(hist, bound, what):
    """every key of the device history within ``bound`` (relative to the key's largest float64 value) of the float64 twin's"""
    for key in hist["f64"]:
        h64, h32, hg = (np.asarray(hist[n][key]) for n in ("f64", "f32", "gpu"))
        assert len(hg) == len(h64)
        d32, dg = np.abs(h32 - h64).max() / np.abs(h64).max(), np.abs(hg - h64).max() / np.abs(h64).max()
        print("%s %s: %s, float32 twin deviation %.3g, device %.3g, bound %.3g" % (what, key, hg, d32, dg, bound))
        assert dg <= bound, (key, hg, h64)


def weight_deviation(params, ref):
    return max(float((a.detach().cpu().double() - r).abs().max() / r.abs().max()) for a, r in zip(params, ref))
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dnn_train_common as S  # noqa: E402
sys.path.pop(0)

from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu
DNN_BF16_PROBA_TOL = 8e-3            # predict against forward_exact("float64"), trained weights: tests/test_nn_gpu.py


@pytest.fixture(scope="module")
def D(rml):
    import radar_ml_amd.dnn as D
    return D


def device_case(shape, contiguous=False):
    import torch
    c = S.case(*shape)
    m = S.make_model(shape[0], shape[1], shape[3], c["seed"], device="cuda")
    if contiguous:
        m = m.to(memory_format=torch.contiguous_format)
    return c, m, S.DeviceStep(m, c["xs"], c["y"], c["cw"])


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_step_against_twin(D, shape):
    from radar_ml_amd import _lib
    c, m, dev = device_case(shape)
    bound = 8.0 * S.e32()
    for rate in S.RATES:
        ref = c["t64"][rate]
        loss, correct, status = dev.run(c["rows"], S.SEED, S.STEP, rate, _lib.DNN_TRAIN)
        errs = S.grad_errors(dev.grads, ref["grads"])
        lerr = abs(loss - ref["loss_sum"]) / abs(ref["loss_sum"])
        print("%s rate %g: loss error %.3g, gradient errors %.3g .. %.3g (worst: tensor %d), E32 %.3g, bound %.3g"
              % (shape, rate, lerr, min(errs), max(errs), int(np.argmax(errs)), S.e32(), bound))
        assert status == 0 and correct == ref["correct"]
        assert lerr <= bound
        assert max(errs) <= bound, errs
        assert dev.guards_intact()


def test_contiguous_kernels_and_no_class_weight(D):
    """the second convolution kernels in (out, in, ky, kx) order (k2_layout 0), gradients in that layout; class_weight NULL = ones"""
    import torch
    from radar_ml_amd import _lib
    shape = (12, 20, 3, 5)
    c, m, dev = device_case(shape, contiguous=True)
    assert dev.layout == 0 and S.DeviceStep(S.make_model(12, 20, 5, c["seed"], device="cuda"), c["xs"], c["y"], None).layout == 1
    loss, correct, status = dev.run(c["rows"], S.SEED, S.STEP, 0.5, _lib.DNN_TRAIN)
    ref = c["t64"][0.5]
    errs = S.grad_errors(dev.grads, ref["grads"])
    assert status == 0 and correct == ref["correct"] and max(errs) <= 8.0 * S.e32(), errs
    plain = S.DeviceStep(m, c["xs"], c["y"], None)
    loss1, _, _ = plain.run(c["rows"], S.SEED, S.STEP, 0.5, _lib.DNN_TRAIN)
    want = S.twin_step(list(m.parameters()), c["xs"], c["y"], c["rows"], None, S.SEED, S.STEP, 0.5, torch.float64)
    assert abs(loss1 - want["loss_sum"]) <= 8.0 * S.e32() * abs(want["loss_sum"])
    assert max(S.grad_errors(plain.grads, want["grads"])) <= 8.0 * S.e32()


@pytest.mark.parametrize("shape", [(20, 12, 7, 3), (80, 80, 37, 3)], ids=["20x12x7", "80x80x37"])
def test_same_call_same_bits(D, shape):
    import torch
    from radar_ml_amd import _lib
    c, m, dev = device_case(shape)
    first = dev.run(c["rows"], S.SEED, S.STEP, 0.5, _lib.DNN_TRAIN)
    g1 = [g.clone() for g in dev.grads]
    for g in dev.grads:
        g.fill_(S.GUARD)
    second = dev.run(c["rows"], S.SEED, S.STEP, 0.5, _lib.DNN_TRAIN)
    assert first == second
    assert all(torch.equal(a, b) for a, b in zip(g1, dev.grads))


@pytest.mark.parametrize("shape", [(12, 20, 3, 5), (80, 80, 37, 3)], ids=["12x20x3", "80x80x37"])
def test_eval_mode(D, shape):
    """no dropout, no gradients; the accumulators ADD; Classifier.evaluate (the Keras surface) is what it was"""
    import torch
    from radar_ml_amd import _lib
    c, m, dev = device_case(shape)
    want = S.twin_step(list(m.parameters()), c["xs"], c["y"], c["rows"], c["cw"], 0, 0, 0.0, torch.float64, train=False)
    loss, correct, status = dev.run(c["rows"], S.SEED, S.STEP, 0.5, _lib.DNN_EVAL)
    print("%s eval: loss error %.3g" % (shape, abs(loss - want["loss_sum"]) / want["loss_sum"]))
    assert status == 0 and correct == want["correct"]
    assert abs(loss - want["loss_sum"]) <= 8.0 * S.e32() * want["loss_sum"]
    assert all(bool((g == S.GUARD).all()) for g in dev.grads) and dev.guards_intact()
    # unweighted, this is evaluate's loss (which clips probabilities at 1e-7: far from these)
    rows = c["rows"].astype(np.int64)
    plain = S.DeviceStep(m, c["xs"], c["y"], None)
    l1, c1, _ = plain.run(c["rows"], 0, 0, 0.0, _lib.DNN_EVAL)
    le, ae = m.evaluate([a[rows] for a in c["xs"]], c["y"][rows], autocast_dtype=None)
    assert abs(l1 / len(rows) - le) <= 1e-5 * max(1.0, le) and c1 / len(rows) == ae


def test_trajectory_20_adam_steps(D):
    """(8, 8) planes, N = 40, batches of 16, 16, 8 reshuffled per epoch: six epochs and two more batches = 20 updates"""
    import torch
    rng = np.random.default_rng(5)
    H = W = 8
    xs = S.grid_planes(rng, 40, H, W)
    y = rng.integers(0, 3, size=40)
    cw = {0: 5.48, 1: 1.26, 2: 1.0}
    perms = [rng.permutation(40).astype(np.int32) for _ in range(6)] + [rng.permutation(40).astype(np.int32)[:32]]
    runs = {}
    for name, hook, device in (("f64", S.TwinTrainer(torch.float64), "cpu"), ("f32", S.TwinTrainer(torch.float32), "cpu"), ("gpu", None, "cuda")):
        m = S.make_model(H, W, 3, 0, device=device).compile(seed=9, **S.ADAM)
        job = m._job(xs, y, None, cw, 16, trusted=True)
        sums = [(hook or D._fit_epoch)(m, job, p)[:2] for p in perms]
        runs[name] = (m, sums, [p.detach().cpu().double() for p in (hook.params if hook else m.parameters())])
    assert runs["gpu"][0]._train_steps == 20 == runs["f64"][0]._train_steps
    ref = runs["f64"][2]
    dev32 = [float((a - r).abs().max() / r.abs().max()) for a, r in zip(runs["f32"][2], ref)]
    devgpu = [float((a - r).abs().max() / r.abs().max()) for a, r in zip(runs["gpu"][2], ref)]
    print("trajectory: float32 twin deviation %.3g .. %.3g, device %.3g .. %.3g" % (min(dev32), max(dev32), min(devgpu), max(devgpu)))
    bound = 8.0 * max(dev32)
    assert max(devgpu) <= bound, (devgpu, dev32)
    moved = [float((r - p.detach().double()).abs().max()) for r, p in zip(ref, S.make_model(H, W, 3, 0).parameters())]
    assert min(moved) > 1e-4                                  # 20 updates of 2e-4 each: every tensor moved
    for (l, c), (l64, c64) in zip(runs["gpu"][1], runs["f64"][1]):
        assert c == c64 and abs(l - l64) <= max(bound, 8.0 * S.e32()) * abs(l64)


def test_bad_rows_and_labels_are_rejected(D):
    """a row index outside [0, N) and a label outside [0, C): status -1 / RadarMLError, nothing written"""
    import torch
    from radar_ml_amd import _lib, RadarMLError
    c, m, dev = device_case((20, 12, 7, 3))
    N = len(c["y"])
    for bad in (N, -1, 2 ** 31 - 1):
        rows = c["rows"].copy()
        rows[3] = bad
        loss, correct, status = dev.run(rows, S.SEED, S.STEP, 0.5, _lib.DNN_TRAIN)
        assert status == -1 and loss == 0.0 and correct == 0
        assert all(bool((g == S.GUARD).all()) for g in dev.grads) and dev.guards_intact()
    for bad in (3, -1):
        y = c["y"].copy()
        y[c["rows"][2]] = bad
        d2 = S.DeviceStep(m, c["xs"], y, c["cw"])
        for mode in (_lib.DNN_TRAIN, _lib.DNN_EVAL):
            assert d2.run(c["rows"], S.SEED, S.STEP, 0.5, mode) == (0.0, 0, -1)
        assert all(bool((g == S.GUARD).all()) for g in d2.grads) and d2.guards_intact()
    # through the public call: an error, and no update
    before = [p.detach().clone() for p in m.parameters()]
    rows = c["rows"].astype(np.int64)
    yb = c["y"][rows].copy()
    yb[0] = 3
    with pytest.raises(RadarMLError, match="status -1"):
        m.train_on_batch([a[rows] for a in c["xs"]], yb)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, m.parameters()))
    loss, acc = m.train_on_batch([a[rows] for a in c["xs"]], c["y"][rows], class_weight=c["cw"])
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and not all(torch.equal(a, b.detach()) for a, b in zip(before, m.parameters()))


def test_fit_end_to_end_and_fresh_weight_packs(D):
    """fit for 3 epochs on 96 samples of 80 x 80 with validation data against the twin; then predict -- the fused bf16 chain, whose
    weight packs are cached on the parameters' version counters -- must see the trained weights, not the packs of the old ones"""
    import copy
    import torch
    rng = np.random.default_rng(11)
    H = W = 80
    xs, vx = S.grid_planes(rng, 96, H, W), S.grid_planes(rng, 32, H, W)
    y, vy = rng.integers(0, 3, size=96), rng.integers(0, 3, size=32)
    cw = {0: 5.48, 1: 1.26, 2: 1.0}
    hist, models = {}, {}
    for name, hook, device in (("f64", S.TwinTrainer(torch.float64), "cpu"), ("f32", S.TwinTrainer(torch.float32), "cpu"), ("gpu", None, "cuda")):
        m = S.make_model(H, W, 3, 0, device=device).compile(seed=21, lr=0.002, beta_1=0.5)
        if name == "gpu":
            old = copy.deepcopy(m)
            p_old = m.predict(vx)                              # builds the weight packs of the untrained model
        with S.hooked(D, hook or D._fit_epoch):
            hist[name] = m.fit(xs, y, batch_size=64, epochs=3, validation_data=(vx, vy), class_weight=cw).history
        models[name] = m
    m = models["gpu"]
    ref = [p.detach().double() for p in models["f64"].parameters()]
    dev32, devg = weight_deviation(models["f32"].parameters(), ref), weight_deviation(m.parameters(), ref)
    print("fit weights: float32 twin deviation %.3g, device %.3g" % (dev32, devg))
    assert devg <= 8.0 * dev32
    history_within(hist, 8.0 * dev32, "fit")
    xg = [torch.from_numpy(a).cuda() for a in vx]
    with torch.no_grad():
        want = m.forward_exact(*xg, precision="float64").cpu().numpy()
        stale = old.forward_exact(*xg, precision="float64").cpu().numpy()
    got = m.predict(vx)
    assert np.abs(got - want).max() <= DNN_BF16_PROBA_TOL
    assert np.abs(got - stale).max() > DNN_BF16_PROBA_TOL and np.abs(p_old - stale).max() <= DNN_BF16_PROBA_TOL
    with torch.no_grad():
        assert np.abs(m.forward_fused(*xg).cpu().numpy() - want).max() <= DNN_BF16_PROBA_TOL


def test_fit_small_batches_larger_validation_set(D):
    """batch_size 16 with 70 validation samples: the validation pass runs in batches of 64 + 6 whatever the training batch is, on the
    one workspace of the fit; history against the twin within 8 x the float32 twin's deviation"""
    import torch
    rng = np.random.default_rng(13)
    H, W = 8, 12
    xs, vx = S.grid_planes(rng, 40, H, W), S.grid_planes(rng, 70, H, W)
    y, vy = rng.integers(0, 3, size=40), rng.integers(0, 3, size=70)
    hist, models = {}, {}
    for name, hook, device in (("f64", S.TwinTrainer(torch.float64), "cpu"), ("f32", S.TwinTrainer(torch.float32), "cpu"), ("gpu", None, "cuda")):
        m = S.make_model(H, W, 3, 0, device=device).compile(seed=4, **S.ADAM)
        with S.hooked(D, hook or D._fit_epoch):
            hist[name] = m.fit(xs, y, batch_size=16, epochs=2, validation_data=(vx, vy), class_weight={0: 5.48, 1: 1.26, 2: 1.0}).history
        models[name] = [p.detach().cpu().double() for p in (hook.params if hook else m.parameters())]
        if name == "gpu":
            assert m._train_steps == 6
            l1, a1 = m.train_on_batch([a[:7] for a in xs], y[:7])           # and a later, smaller job of its own
            assert np.isfinite(l1) and m._train_steps == 7
    dev32, devg = weight_deviation(models["f32"], models["f64"]), weight_deviation(models["gpu"], models["f64"])
    print("fit batch 16 weights: float32 twin deviation %.3g, device %.3g" % (dev32, devg))
    assert devg <= 8.0 * dev32
    history_within(hist, 8.0 * dev32, "fit batch 16")


def test_fit_partial_last_batch_at_many_row_splits(D):
    """40 x 40 planes (H/4 = 10: the backward trunk kernel picks its row splits from the batch), batch_size 16, N = 30: the last batch
    of 14 uses MORE partial-sum slots (14 x 7) than a batch of 16 (16 x 6), on the workspace sized for batch_size; no validation data"""
    import torch
    rng = np.random.default_rng(17)
    H = W = 40
    xs, y = S.grid_planes(rng, 30, H, W), rng.integers(0, 3, size=30)
    hist, models = {}, {}
    for name, hook, device in (("f64", S.TwinTrainer(torch.float64), "cpu"), ("f32", S.TwinTrainer(torch.float32), "cpu"), ("gpu", None, "cuda")):
        m = S.make_model(H, W, 3, 0, device=device).compile(seed=6, **S.ADAM)
        with S.hooked(D, hook or D._fit_epoch):
            hist[name] = m.fit(xs, y, batch_size=16, epochs=2, class_weight={0: 5.48, 1: 1.26, 2: 1.0}).history
        models[name] = [p.detach().cpu().double() for p in (hook.params if hook else m.parameters())]
        assert m._train_steps == 4
    assert sorted(hist["gpu"]) == ["accuracy", "loss"]
    dev32, devg = weight_deviation(models["f32"], models["f64"]), weight_deviation(models["gpu"], models["f64"])
    print("fit 40x40 weights after 4 updates: float32 twin deviation %.3g, device %.3g" % (dev32, devg))
    assert devg <= 8.0 * dev32
    history_within(hist, 8.0 * dev32, "fit 40x40 batch 16 + 14")


def test_bench_tool_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dnn_train_bench.py"), "--torch", "--samples", "128", "--steps", "3",
                          "--warmup", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, check=True).stdout.decode()
    r = json.loads(out.strip().splitlines()[-1])
    assert r["step_ms"] > 0 and r["call_ms"] > 0 and r["epoch_ms"] > 0 and r["torch_step_ms"] > 0 and r["batch"] == 64 and r["planes"] == [80, 80]
