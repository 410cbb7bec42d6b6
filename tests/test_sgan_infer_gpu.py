"""SGAN classifier inference on the fused HIP chain (csrc/sgan_infer.hip + the LeakyReLU tail of csrc/dense.hip) against the plain
PyTorch inference path in float32.  The tolerance is measured, not chosen: what bf16 autocast costs the plain path against float32 on
the same weights and planes (sgan_infer_common.yardstick: E_feat on the flattened trunk output, E_p on the probabilities); the fused
chain has to stay within twice that (the project's precedent: test_g_step_gradients_fused_against_float32)."""
import importlib

import numpy as np
import pytest
import torch

from sgan_infer_common import (SLOPE, case, check_labels, feat_error, make_model, make_planes, plain_eval, synth_frames, yardstick)

pytestmark = pytest.mark.gpu

RML_ERR_UNSUPPORTED = -2
DENSE_TAIL_BOUND = 2e-5         # test_nn_gpu.py test_fused_dense_tail_vs_float64: the relu tail against float64 on the same bf16 operands
PREPROCESS_ALLOWANCE = 2e-4     # test_nn_gpu.py test_predict_volumes_fused_and_exact_preprocessing_agree: fused against exact preprocessing


@pytest.fixture(scope="module")
def sgan(rml):
    return importlib.import_module("radar_ml_amd.sgan")


@pytest.mark.parametrize("B", [1, 3, 9, 33])
@pytest.mark.parametrize("H,W", [(8, 8), (16, 16), (16, 40), (40, 16)])
def test_trunk_against_float32(sgan, H, W, B):
    """features_fused against the plain float32 layers: within 2 x E_feat; float32 and bfloat16 planes give identical bits"""
    _check_trunk(H, W, B)


@pytest.mark.parametrize("B", [2, 9])
def test_trunk_against_float32_default_size(sgan, B):
    _check_trunk(128, 128, B)


def _check_trunk(H, W, B):
    e_feat, _ = yardstick()
    seed = {(8, 8): 1, (16, 16): 2, (16, 40): 3, (40, 16): 4, (128, 128): 5}[(H, W)]
    model, xs_all, fv_all, _ = case(H, W, 33 if H < 128 else 9, 3, seed)
    xs, ref = [x[:B] for x in xs_all], fv_all[:B]
    got = model.features_fused(*xs)
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    err = feat_error(got.float(), ref)
    print("trunk %dx%d B=%d: fused max|d|/max|ref| = %.3e (bound 2 x E_feat = %.3e)" % (H, W, B, err, 2 * e_feat))
    assert err <= 2 * e_feat
    got16 = model.features_fused(*[x.to(torch.bfloat16) for x in xs])
    assert torch.equal(got, got16)
    got4 = model.features_fused(*[x.unsqueeze(1) for x in xs])             # (N, 1, H, W) planes are taken as they are
    assert torch.equal(got, got4)


@pytest.mark.parametrize("H,W,B", [(16, 16, 2100), (128, 128, 70)])
def test_trunk_over_more_than_one_round(sgan, H, W, B):
    """Batches whose tiles do not fit one round of the persistent layer-1/2 kernel (eight tiles per workgroup, one workgroup per CU and
    branch): the second round takes the other LDS stage parity, its first weight slab is the one prefetched behind the last tap of the
    first round, and its last workgroups are partly or wholly past the end.  Against the plain float32 layers, and the samples on both
    sides of the round boundary and the last one against the same samples in a small batch (first round only): the same bits."""
    e_feat, e_p = yardstick()
    tiles = ((H // 4) * (W // 4) + 31) // 32
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert B * tiles > 8 * n_cu and (B * tiles) % (8 * n_cu) != 0, "the case no longer reaches a second, partly filled round"
    model = make_model(H, W, 3, seed=51, device="cuda")
    xs = make_planes(B, H, W, seed=52, device="cuda")
    fv_ref, p_ref = plain_eval(model, xs)
    fv = model.features_fused(*xs)
    p = model.dense_tail_fused(fv)
    e_f, e_pr = feat_error(fv.float(), fv_ref), float((p - p_ref).abs().max())
    print("two rounds %dx%d B=%d: fused max|d|/max|ref| = %.3e (bound %.3e), |dp| = %.3e (bound %.3e)" % (H, W, B, e_f, 2 * e_feat, e_pr, 2 * e_p))
    assert e_f <= 2 * e_feat and e_pr <= 2 * e_p
    # per sample too: an error confined to the second round's samples must not hide behind the batch's largest feature
    per = (fv.float() - fv_ref).abs().amax(dim=1) / fv_ref.abs().amax(dim=1)
    assert float(per.max()) <= 2 * e_feat
    assert torch.equal(fv, model.features_fused(*[x.to(torch.bfloat16) for x in xs]))
    edge = (8 * n_cu + tiles - 1) // tiles              # the first sample with a tile in the second round
    idx = torch.tensor([edge - 1, edge, min(edge + 1, B - 1), B - 1, 0], device="cuda")
    sub = [x[idx] for x in xs]
    assert torch.equal(model.features_fused(*sub), fv[idx]) and torch.equal(model.forward_fused(*sub), p[idx])


@pytest.mark.parametrize("H,W,N", [(16, 40, 33), (128, 128, 9)])
def test_a_row_is_a_function_of_the_row(sgan, H, W, N):
    """a sample's features and probabilities are the same bits alone, as the first, middle and last of a batch, in a permuted batch and
    on a second call (no atomics, fixed summation orders)"""
    model, xs, _, _ = case(H, W, N, 3, 3 if H == 16 else 5)
    fv = model.features_fused(*xs)
    p = model.dense_tail_fused(fv)
    assert torch.equal(fv, model.features_fused(*xs)) and torch.equal(p, model.forward_fused(*xs))
    for i in (0, N // 2, N - 1):
        one = [x[i:i + 1] for x in xs]
        assert torch.equal(model.features_fused(*one)[0], fv[i])
        assert torch.equal(model.forward_fused(*one)[0], p[i])
        others = [j for j in range(N) if j != i][:4]
        for pos in (0, 2, 4):                       # first, middle, last of a batch of five
            idx = torch.tensor(others[:pos] + [i] + others[pos:], device="cuda")
            sub = [x[idx] for x in xs]
            assert torch.equal(model.features_fused(*sub)[pos], fv[i])
            assert torch.equal(model.forward_fused(*sub)[pos], p[i])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(4)).cuda()
    xp = [x[perm] for x in xs]
    assert torch.equal(model.features_fused(*xp), fv[perm]) and torch.equal(model.forward_fused(*xp), p[perm])


def _tail_operands(K, N, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(s, device="cuda", generator=g)
    x = r(N, K)
    fv = torch.where(x > 0, x, SLOPE * x).to(torch.bfloat16)
    w1 = (r(64, K) / K ** 0.5).to(torch.bfloat16)
    b1, w2, b2 = r(64) * 0.1, r(64, 64) / 8.0, r(64) * 0.1
    w3, b3 = r(C, 64) / 4.0, r(C) * 0.1
    return fv, w1, b1, w2, b2, w3, b3


def _tail_float64(fv, w1, b1, w2, b2, w3, b3, act):
    h = act(fv.double() @ w1.double().t() + b1.double())
    h = act(h @ w2.double().t() + b2.double())
    return torch.softmax(h @ w3.double().t() + b3.double(), dim=-1)


@pytest.mark.parametrize("C", [2, 3, 16])
@pytest.mark.parametrize("N", [1, 5, 130])
@pytest.mark.parametrize("K", [192, 24576])
def test_lrelu_dense_tail_vs_float64(rml, K, N, C):
    """rml_dense_tail_lrelu against the float64 layers on the same bf16-rounded operands, within the bound the CNN's relu tail is held
    to; rml_dnn_dense_tail on the same inputs still is the relu tail (same bound against the float64 relu layers), its split-K partial
    sums -- the shared k_fc1_splitk -- are the very bits the LeakyReLU entry point leaves in its workspace, and both are deterministic"""
    from radar_ml_amd import _lib
    lib, ctx = _lib.load(), _lib.context(torch.device("cuda", torch.cuda.current_device()))
    fv, w1, b1, w2, b2, w3, b3 = _tail_operands(K, N, C, seed=K + 7 * N + C)
    w2t = w2.t().contiguous()
    nbytes = int(lib.rml_dnn_dense_workspace_bytes(ctx, N, K))
    st = _lib.stream_ptr(fv.device)

    def run(lrelu):
        ws = torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda")
        out = torch.empty((N, C), dtype=torch.float32, device="cuda")
        if lrelu:
            rc = lib.rml_dense_tail_lrelu(ctx, _lib.ptr(fv), K, N, K, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2t), _lib.ptr(b2), _lib.ptr(w3),
                                          _lib.ptr(b3), C, SLOPE, _lib.ptr(ws), nbytes, _lib.ptr(out), st)
        else:
            rc = lib.rml_dnn_dense_tail(ctx, _lib.ptr(fv), K, 0, N, K, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2t), _lib.ptr(b2), _lib.ptr(w3),
                                        _lib.ptr(b3), C, _lib.ptr(ws), nbytes, _lib.ptr(out), st)
        _lib.check(rc, "dense tail")
        torch.cuda.synchronize()
        return out, ws

    got, ws_l = run(True)
    want = _tail_float64(fv, w1, b1, w2, b2, w3, b3, lambda t: torch.where(t > 0, t, SLOPE * t))
    e_l = float((got.double() - want).abs().max())
    relu, ws_r = run(False)
    want_r = _tail_float64(fv, w1, b1, w2, b2, w3, b3, torch.relu)
    e_r = float((relu.double() - want_r).abs().max())
    print("tail K=%d N=%d C=%d: LeakyReLU |dp| = %.2e, relu |dp| = %.2e (bound %.0e)" % (K, N, C, e_l, e_r, DENSE_TAIL_BOUND))
    assert e_l < DENSE_TAIL_BOUND and e_r < DENSE_TAIL_BOUND
    assert torch.allclose(got.sum(1), torch.ones(N, device="cuda"), atol=1e-5)
    assert torch.equal(ws_l, ws_r)                      # the first layer's partial sums: one kernel behind both entry points
    again, _ = run(True)
    again_r, _ = run(False)
    assert torch.equal(got, again) and torch.equal(relu, again_r)
    assert float((got - relu).abs().max()) > 1e-4       # and the two activations are two functions


@pytest.mark.parametrize("H,W,B,C,seed", [(16, 16, 7, 3, 7), (128, 128, 5, 3, 5), (128, 128, 5, 5, 6)])
def test_forward_fused_end_to_end(sgan, H, W, B, C, seed):
    """forward_fused: probabilities within 2 x E_p of the plain float32 layers; every row outside the near-tie gap has the float32 label"""
    _, e_p = yardstick()
    model, xs, _, p_ref = case(H, W, B if (H, C) != (128, 3) else 9, C, seed)
    xs, p_ref = [x[:B] for x in xs], p_ref[:B]
    p = model.forward_fused(*xs)
    assert p.dtype == torch.float32 and p.shape == (B, C) and p.is_cuda
    err = float((p - p_ref).abs().max())
    print("forward_fused %dx%d B=%d C=%d: max |dp| = %.3e (bound 2 x E_p = %.3e)" % (H, W, B, C, err, 2 * e_p))
    assert err <= 2 * e_p
    assert torch.allclose(p.sum(1), torch.ones(B, device="cuda"), atol=1e-5)
    check_labels(p, p_ref, e_p, "forward_fused %dx%d C=%d" % (H, W, C))
    assert torch.equal(p, model.forward_fused(*[x.to(torch.bfloat16) for x in xs]))


@pytest.mark.parametrize("grid", [(22, 31, 176), (64, 64, 128)])
def test_predict_volumes(rml, sgan, grid):
    """volumes -> probabilities against projection (rml_project) -> Pillow-exact resize in float32 -> plain float32 layers: exact_resize
    within 2 x E_p, the fused preprocessing within that plus the CNN chain's preprocessing allowance; uint8 and float32 volumes of the
    same frames: the same bits; a frame off the integer grid in the batch: every row still right; the pass size changes no bit"""
    nc = importlib.import_module("radar_ml_amd.nn_common")
    _, e_p = yardstick()
    model = case(128, 128, 9, 3, 5)[0]
    vol = synth_frames(6, grid, seed=21)
    v = torch.from_numpy(vol).cuda()

    def reference(vv):
        feat = rml.process_volumes(vv, mode="max", scale=False)
        return plain_eval(model, nc.preprocess_features(feat, grid, (128, 128), out_dtype="float32"))[1]

    # the Walabot grid takes the fused preprocessing kernel; 64 x 64 x 128 at 128 x 128 does not fit its LDS layout (the header's rule
    # is necessary, not sufficient: rml_dnn_preprocess_supported answers) and goes through the exact resize either way
    assert nc.preprocess_supported(grid, (128, 128)) == (grid == (22, 31, 176))
    p_ref = reference(v)
    exact = model.predict_volumes(v, exact_resize=True, return_numpy=False)
    fused = model.predict_volumes(v, return_numpy=False)
    e_exact, e_fused = float((exact - p_ref).abs().max()), float((fused - p_ref).abs().max())
    print("predict_volumes %s: exact preprocessing |dp| = %.3e, fused preprocessing |dp| = %.3e (2 x E_p = %.3e)" % (grid, e_exact, e_fused, 2 * e_p))
    assert e_exact <= 2 * e_p
    assert e_fused <= 2 * e_p + PREPROCESS_ALLOWANCE
    check_labels(fused, p_ref, e_p, "predict_volumes %s" % (grid,))
    as_numpy = model.predict_volumes(vol)                                   # host float32 volumes in, numpy out
    assert isinstance(as_numpy, np.ndarray) and as_numpy.dtype == np.float32 and np.array_equal(as_numpy, fused.cpu().numpy())
    v8 = v.to(torch.uint8)
    assert torch.equal(model.predict_volumes(v8, return_numpy=False), fused)
    assert torch.equal(model.predict_volumes(v8, exact_resize=True, return_numpy=False), exact)
    for bs in (4, 6):
        assert torch.equal(model.predict_volumes(v8, batch_size=bs, return_numpy=False), fused)
    v2 = v.clone()
    v2[3] *= 0.731                                                          # returns that are no integers: that frame leaves the code grid
    p2_ref = reference(v2)
    p2 = model.predict_volumes(v2, return_numpy=False)
    assert float((p2 - p2_ref).abs().max()) <= 2 * e_p + PREPROCESS_ALLOWANCE
    keep = [0, 1, 2, 4, 5]
    assert float((p2[keep] - fused[keep]).abs().max()) <= PREPROCESS_ALLOWANCE


def test_packs_are_fresh_after_a_training_step(sgan):
    """predict(fused=True), one train_on_batch_c, predict(fused=True) again: the second result is the NEW weights' (within 2 x E_p of
    the plain float32 layers on them) and differs from the first by more than that"""
    _, e_p = yardstick()
    model = make_model(16, 16, 3, seed=31, device="cuda")
    # bfloat16 autocast: no loss scale, so the one step is never skipped for an overflow; the rate is large so that the step moves the
    # probabilities by far more than the tolerance (Adam's first step moves every weight by the rate)
    trainer = sgan.DiscriminatorTrainer(model, lr=5e-2, amp_dtype="bfloat16")
    xs = [x.cpu().numpy() for x in make_planes(8, 16, 16, seed=32)]
    y = np.arange(8) % 3
    p1 = trainer.predict(xs, fused=True)
    assert float(np.abs(p1 - plain_eval(model, [torch.from_numpy(x).cuda() for x in xs])[1].cpu().numpy()).max()) <= 2 * e_p
    trainer.train_on_batch_c(xs, y)
    p2 = trainer.predict(xs, fused=True)
    ref2 = plain_eval(model, [torch.from_numpy(x).cuda() for x in xs])[1].cpu().numpy()
    print("after one step: |p2 - float32(new weights)| = %.3e, |p2 - p1| = %.3e (2 x E_p = %.3e)"
          % (float(np.abs(p2 - ref2).max()), float(np.abs(p2 - p1).max()), 2 * e_p))
    assert float(np.abs(p2 - ref2).max()) <= 2 * e_p
    assert float(np.abs(p2 - p1).max()) > 2 * e_p
    loss, acc = trainer.evaluate(xs, y, fused=True)
    loss_p, acc_p = trainer.evaluate(xs, y)
    assert np.isfinite(loss) and abs(loss - loss_p) < 0.1 and 0.0 <= acc <= 1.0


def test_packs_are_fresh_after_a_graph_replayed_step(sgan):
    """The same with ``use_graph=True``: after three eager steps forward + backward are replayed from a captured graph, and a replay
    bumps no version counter (not even num_batches_tracked's): the packs' freshness then rests on DeviceAdam.step telling torch about
    the parameters it wrote.  After a replayed step the fused prediction is the new weights'."""
    _, e_p = yardstick()
    model = make_model(16, 16, 3, seed=33, device="cuda")
    trainer = sgan.DiscriminatorTrainer(model, lr=1e-2, amp_dtype="bfloat16", use_graph=True)
    xs = [x.cpu().numpy() for x in make_planes(8, 16, 16, seed=34)]
    y = np.arange(8) % 3
    for _ in range(4):                                  # three eager warm-up steps, then capture + first replay
        trainer.train_on_batch_c(xs, y)
    assert "graph" in trainer._graphs["c"]
    trainer.predict(xs, fused=True)
    packs = model.folded_packs()
    w_before = model.fc3.weight.detach().clone()
    trainer.train_on_batch_c(xs, y)                     # a replayed step
    assert not torch.equal(model.fc3.weight.detach(), w_before)
    p = trainer.predict(xs, fused=True)
    assert model.folded_packs() is not packs
    ref = plain_eval(model, [torch.from_numpy(x).cuda() for x in xs])[1].cpu().numpy()
    print("after a replayed step: |p - float32(new weights)| = %.3e (2 x E_p = %.3e)" % (float(np.abs(p - ref).max()), 2 * e_p))
    assert float(np.abs(p - ref).max()) <= 2 * e_p


def test_keras_round_trip_gives_the_same_bits(sgan):
    """set_keras_weights(*other.keras_weights()) into a fresh model: bit-identical forward_fused"""
    other, xs, _, _ = case(16, 16, 7, 3, 7)
    fresh = sgan.Discriminator(((16, 16, 1),) * 3, 3).to("cuda").eval()
    before = fresh.forward_fused(*xs)
    fresh.set_keras_weights(*other.keras_weights())
    after = fresh.forward_fused(*xs)
    assert torch.equal(after, other.forward_fused(*xs)) and not torch.equal(after, before)


def test_unsupported_planes_raise(sgan):
    """12 x 16 planes: forward_fused raises, the C call returns RML_ERR_UNSUPPORTED and writes nothing, predict(fused=True) names the size"""
    from radar_ml_amd import _lib
    model = make_model(12, 16, 3, seed=41, device="cuda")
    xs = make_planes(2, 12, 16, seed=42, device="cuda")
    assert plain_eval(model, xs)[1].shape == (2, 3)                          # the plain layers take the size
    with pytest.raises(ValueError, match="12x16"):
        model.forward_fused(*xs)
    with pytest.raises(ValueError, match="12x16"):
        sgan.DiscriminatorTrainer(model).predict([x.cpu().numpy() for x in xs], fused=True)
    lib = _lib.load()
    pk = make_model(16, 16, 3, seed=43, device="cuda").folded_packs()
    feat = torch.full((2, 4 * 96), 7.0, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros((1 << 20,), dtype=torch.uint8, device="cuda")
    rc = lib.rml_sgan_trunk(_lib.context(feat.device), _lib.ptr(xs[0]), _lib.ptr(xs[1]), _lib.ptr(xs[2]), 0, 2, 12, 16, _lib.ptr(pk["w1"]),
                            _lib.ptr(pk["b1"]), _lib.ptr(pk["w2t"]), _lib.ptr(pk["b2"]), _lib.ptr(pk["w3t"]), _lib.ptr(pk["b3"]), SLOPE,
                            _lib.ptr(feat), _lib.ptr(ws), int(ws.numel()), _lib.stream_ptr(feat.device))
    torch.cuda.synchronize()
    assert rc == RML_ERR_UNSUPPORTED and b"12x16" in lib.rml_last_error()
    assert bool((feat == 7.0).all()) and int(ws.count_nonzero()) == 0        # no kernel ran
