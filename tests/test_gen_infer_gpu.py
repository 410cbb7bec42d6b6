"""The SGAN generator's inference on the fused HIP chain (csrc/gen_infer.hip + the forward of csrc/gen.hip).  ``rml_gen_up_forward``
against the float64 twin on the same half-rounded operands, with a per-element bound from the kernel's own arithmetic; the whole chain
against the plain PyTorch layers in float32, within twice what the plain layers under the same autocast type cost against float32
(gen_infer_common.yardstick, measured at run time); determinism, the keywords, the freshness of the packs, the error paths."""
import importlib
import pickle

import numpy as np
import pytest
import torch

from gen_infer_common import (CHAIN_CASES, case, image_error, in_band, make_generator, make_latent, plain_eval, twin_up, twin_up_linear,
                              yardstick)

pytestmark = pytest.mark.gpu

DTYPES = {"bfloat16": (torch.bfloat16, 1, 2.0 ** -8), "float16": (torch.float16, 0, 2.0 ** -11)}
# (N, H, W): one tile, a batch of tiles, 2 x 2 tiles, one row / one column of tiles, more than one tile in both directions with
# different counts, the largest plane, an odd batch
UP_SHAPES = ((1, 8, 8), (3, 8, 8), (2, 16, 16), (1, 8, 24), (1, 24, 8), (2, 24, 40), (1, 128, 128), (5, 16, 16))
C = 128


@pytest.fixture(scope="module")
def sgan(rml):
    return importlib.import_module("radar_ml_amd.sgan")


def _operands(N, H, W, dtype, seed):
    """x (N, H, W, C), wt (4, C, 4C) rounded to ``dtype``, bias (C) float32, on the GPU: x non-zero everywhere (borders included), wt
    non-zero but for the few draws that float16 flushes to zero"""
    g = torch.Generator().manual_seed(5000 + seed)
    x = torch.randn((N, H, W, C), generator=g).to(dtype)
    wt = (torch.randn((4, C, 4 * C), generator=g) / (4 * C) ** 0.5 * 2.0 ** 0.5).to(dtype)
    bias = torch.randn((C,), generator=g) * 0.2
    assert bool((x != 0).all()) and float((wt != 0).float().mean()) > 0.999
    return x.cuda(), wt.cuda(), bias.cuda()


def _gen_up(x, wt, bias, code):
    from radar_ml_amd import _lib
    lib = _lib.load()
    N, H, W, _ = x.shape
    y = torch.full((N, 2 * H, 2 * W, C), float("nan"), dtype=x.dtype, device=x.device)
    _lib.check(lib.rml_gen_up_forward(_lib.context(x.device), _lib.ptr(x), code, N, H, W, C, _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(y),
                                      _lib.stream_ptr(x.device)), "rml_gen_up_forward")
    return y


@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("dtype_name", sorted(DTYPES))
def test_gen_up_against_the_twin(rml, dtype_name, shape):
    """|kernel - twin| <= 514 * 2^-24 * (sum |x w| + |b|) + u |y| per element: 512 products and the bias accumulated in float32 (each
    of the 513 additions and the final rounding of the sum at most half an ulp of a partial sum that sum |x w| + |b| bounds, with
    room for the order inside the matrix core), then one rounding to the half type (u = 2^-8 for bfloat16, 2^-11 for float16)"""
    dtype, code, u = DTYPES[dtype_name]
    N, H, W = shape
    x, wt, bias = _operands(N, H, W, dtype, seed=H * 1000 + W * 10 + N)
    got = _gen_up(x, wt, bias, code).double().cpu().numpy()
    xn, wn, bn = x.double().cpu().numpy(), wt.double().cpu().numpy(), bias.double().cpu().numpy()
    ref = twin_up(xn, wn, bn)
    mag = twin_up_linear(np.abs(xn), np.abs(wn), np.abs(bn))
    bound = 514.0 * 2.0 ** -24 * mag + u * np.abs(ref)
    assert got.shape == ref.shape == (N, 2 * H, 2 * W, C) and np.isfinite(got).all()
    ratio = float((np.abs(got - ref) / bound).max())
    print("gen_up %s %s: max error / bound = %.3f (max |y| = %.2f, %.1f %% of the outputs positive)" % (
        dtype_name, shape, ratio, float(np.abs(ref).max()), 100.0 * float((ref > 0).mean())))
    assert ratio <= 1.0


@pytest.mark.parametrize("dtype_name", sorted(DTYPES))
def test_gen_up_deterministic_and_batch_independent(rml, dtype_name):
    dtype, code, _ = DTYPES[dtype_name]
    x, wt, bias = _operands(5, 16, 16, dtype, seed=77)
    y5 = _gen_up(x, wt, bias, code)
    assert torch.equal(y5.view(torch.int16), _gen_up(x, wt, bias, code).view(torch.int16))          # a second call
    for pos in (0, 4):
        alone = _gen_up(x[pos:pos + 1].contiguous(), wt, bias, code)
        assert torch.equal(alone[0].view(torch.int16), y5[pos].view(torch.int16)), "sample %d differs alone and in the batch" % pos


@pytest.mark.parametrize("dtype_name", sorted(DTYPES))
@pytest.mark.parametrize("cs", CHAIN_CASES, ids=lambda c: "L%d_C%d_b%d_up%d_B%d_s%d" % c)
def test_chain_against_float32(sgan, cs, dtype_name):
    dtype = DTYPES[dtype_name][0]
    tol = 2.0 * yardstick(dtype_name)
    model, z, ref = case(*cs)
    B, S = cs[4], cs[2] * 2 ** cs[3]
    frac = in_band(ref)
    assert frac >= 0.5, "the test model gives flat or saturated images (%.2f of the pixels in [0.05, 0.95])" % frac
    got = model.forward_fused(z, dtype=dtype)
    assert len(got) == 3
    for v in got:
        assert v.dtype == torch.float32 and tuple(v.shape) == (B, 1, S, S) and v.is_cuda and float(v.abs().max()) <= 1.0
    err = image_error(got, ref)
    print("chain %s %s: max |fused - float32| = %.3e (bound 2 E = %.3e)" % (cs, dtype_name, err, tol))
    assert err <= tol
    again = model.forward_fused(z, dtype=dtype)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_chain_batch_independent(sgan):
    model, z, _ = case(*CHAIN_CASES[5])                # n_up = 2, B = 9
    full = model.forward_fused(z)
    for pos in (0, 4):
        alone = model.forward_fused(z[pos:pos + 1])
        assert all(torch.equal(a[0], f[pos]) for a, f in zip(alone, full))


def test_predict_keyword(sgan):
    model, z, _ = case(*CHAIN_CASES[1])                # n_up = 1, B = 3
    want = model.forward_fused(z)
    plain_np, plain_t = model.predict(z), model.predict(z, return_numpy=False)
    got_np, got_t = model.predict(z, fused=True), model.predict(z, return_numpy=False, fused=True)
    for w, pn, pt, gn, gt in zip(want, plain_np, plain_t, got_np, got_t):
        assert isinstance(gn, np.ndarray) and gn.shape == pn.shape == (3, 16, 16, 1) and gn.dtype == pn.dtype == np.float32
        assert gt.shape == pt.shape and gt.dtype == pt.dtype and gt.device == pt.device and gt.is_contiguous()
        assert torch.equal(gt, w) and np.array_equal(gn, w.permute(0, 2, 3, 1).cpu().numpy())
    f16 = model.predict(z, return_numpy=False, fused=True, amp_dtype=torch.float16)
    assert all(torch.equal(a, b) for a, b in zip(f16, model.forward_fused(z, dtype=torch.float16)))
    assert not torch.equal(f16[0], got_t[0])
    with pytest.raises(ValueError):
        model.forward_fused(z.clone().requires_grad_(True))
    assert model.predict(z[:0], fused=True)[0].shape == (0, 16, 16, 1)


def test_generate_fake_samples_draws(sgan):
    model, _, _ = case(*CHAIN_CASES[1])
    ra, rb = np.random.default_rng(5), np.random.default_rng(5)
    xa, ya = sgan.generate_fake_samples(model, 16, 4, ra, return_numpy=False, fused=True)
    xb, yb = sgan.generate_fake_samples(model, 16, 4, rb, return_numpy=False, fused=False)
    assert np.array_equal(ya, yb) and ra.bit_generator.state == rb.bit_generator.state
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(xa, xb))
    assert image_error(xa, xb) <= 2.0 * yardstick("bfloat16")


def test_data_product(sgan, tmp_path):
    from radar_ml_amd.nn_common import resize_bicubic
    datasets = importlib.import_module("radar_ml_amd.datasets")
    model, _, _ = case(*CHAIN_CASES[4])                # n_up = 2: 32 x 32 images
    sizes = (sgan.XZ_SIZE, sgan.YZ_SIZE, sgan.XY_SIZE)

    def expected(zs):
        imgs = model.forward_fused(torch.as_tensor(zs))
        return [resize_bicubic((255.0 * (v[:, 0] + 1.0) / 2.0).contiguous(), (rows, cols), scale=False).cpu().numpy()
                for v, (cols, rows) in zip(imgs, sizes)]

    z5 = sgan.generate_latent_points(16, 5, np.random.default_rng(9))
    want = expected(z5)
    got = sgan.generated_samples(model, 16, 5, np.random.default_rng(9), fused=True)
    assert len(got) == 5
    for i, s in enumerate(got):
        for pl, w, (cols, rows) in zip(s, want, sizes):
            assert pl.shape == (rows, cols) and pl.dtype == np.float32 and np.array_equal(pl, w[i])
    # the data set in batches of 2: the latent points are drawn batch by batch
    rng = np.random.default_rng(9)
    want_b = [expected(sgan.generate_latent_points(16, nb, rng)) for nb in (2, 2, 1)]
    want_b = [np.concatenate([w[k] for w in want_b]) for k in range(3)]
    ds = sgan.generate_dataset(model, 5, latent_dim=16, rng=np.random.default_rng(9), batch_size=2)
    assert len(ds) == 5 and all(np.array_equal(ds[i][k], want_b[k][i]) and ds[i][k].dtype == np.float32 for i in range(5) for k in range(3))
    path = str(tmp_path / "generated_data_0001.pickle")
    assert sgan.generate_dataset(model, 5, latent_dim=16, rng=np.random.default_rng(9), batch_size=2, path=path) == 5
    xz, yz, xy, labels = datasets.load_dataset(path)
    assert labels == ["generated_data"] * 5 and xz.shape == (5, 22, 176) and yz.shape == (5, 31, 176) and xy.shape == (5, 22, 31)
    for k, arr in enumerate((xz, yz, xy)):
        assert arr.dtype == np.float32 and np.array_equal(arr, want_b[k])
    with open(path, "rb") as fp:
        assert set(pickle.load(fp)) == {"samples", "labels"}
    plain = sgan.generate_dataset(model, 3, latent_dim=16, rng=np.random.default_rng(9), fused=False)
    assert len(plain) == 3 and plain[0][0].shape == (22, 176)


@pytest.mark.parametrize("device_adam", [True, False])
def test_packs_fresh_after_a_g_step(sgan, device_adam, monkeypatch):
    """one ``GanTrainer.train_on_batch_g`` step (the fused training forward advances the moving statistics through raw pointers; the
    update is DeviceAdam's or torch's): the next fused call runs on the updated model"""
    monkeypatch.setenv("RML_DEVICE_ADAM", "1" if device_adam else "0")
    tol = 2.0 * yardstick("bfloat16")
    gen = make_generator(16, 128, 8, 1, seed=91, device="cuda")
    disc = sgan.Discriminator(((16, 16, 1),) * 3, 3).to("cuda").to(memory_format=torch.channels_last)
    dt = sgan.DiscriminatorTrainer(disc, amp_dtype="float16", ddp=False)
    assert (dt._dev_adam is not None) == device_adam
    gan = sgan.GanTrainer(gen, dt, lr=0.02)
    z = make_latent(6, 16, seed=92, device="cuda")
    before = gen.forward_fused(z)
    key = gen.packs_key()
    assert image_error(before, plain_eval(gen, z)) <= tol
    loss = gan.train_on_batch_g(make_latent(8, 16, seed=93, device="cuda"), np.full((8, 1), 0.9))
    assert np.isfinite(loss) and gen.packs_key() != key
    gen.eval()
    after = gen.forward_fused(z)
    moved, err = image_error(after, before), image_error(after, plain_eval(gen, z))
    print("g step (DeviceAdam %s): the fused images moved by %.3e, against the plain float32 layers of the updated model %.3e "
          "(bound %.3e)" % (device_adam, moved, err, tol))
    assert moved > 4.0 * tol and err <= tol


def test_keras_round_trip_gives_the_same_bits(sgan):
    gen = make_generator(16, 128, 8, 2, seed=95, device="cuda")
    z = make_latent(3, 16, seed=95, device="cuda")
    a = gen.forward_fused(z)
    key = gen.packs_key()
    gen.set_keras_weights(gen.keras_weights())
    assert gen.packs_key() != key
    assert all(torch.equal(x, y) for x, y in zip(a, gen.forward_fused(z)))


def test_unsupported_geometry_raises(sgan):
    gen = make_generator(5, 8, 8, 2, seed=96, device="cuda")
    z = make_latent(2, 5, seed=96, device="cuda")
    with pytest.raises(ValueError):
        gen.predict(z, fused=True)
    with pytest.raises(ValueError):
        sgan.generated_samples(gen, 5, 2, np.random.default_rng(0), fused=True)
    out = gen.predict(z, fused=False)
    assert out[0].shape == (2, 32, 32, 1) and np.isfinite(out[0]).all()


def test_workspace_one_byte_short_writes_nothing(sgan):
    from radar_ml_amd import _lib
    lib = _lib.load()
    model, z, _ = case(*CHAIN_CASES[1])
    pk = model.generator_packs(torch.bfloat16)
    n = int(z.shape[0])
    nbytes = int(lib.rml_sgan_generate_workspace_bytes(n, 8, 1, 128))
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    outs = [torch.full((n, 16, 16), 7.0, device="cuda") for _ in range(3)]

    def call(nb, C_=128):
        return lib.rml_sgan_generate(_lib.context(z.device), _lib.ptr(z), n, 16, 8, 1, C_, 1, _lib.ptr(pk["dense_w"]), _lib.ptr(pk["dense_b"]),
                                     _lib.ptr(pk["up_wt"]), _lib.ptr(pk["up_bias"]), _lib.ptr(pk["out_w"]), _lib.ptr(pk["out_b"]),
                                     _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(ws), nb, _lib.stream_ptr(z.device))
    rc = call(nbytes - 1)
    torch.cuda.synchronize()
    assert rc == -1 and b"workspace" in lib.rml_last_error()
    assert all(bool((o == 7.0).all()) for o in outs) and not bool(ws.any())
    assert call(nbytes, C_=64) == -2                   # RML_ERR_UNSUPPORTED, before any launch
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    assert call(nbytes) == 0
    torch.cuda.synchronize()
    want = model.forward_fused(z)
    assert all(torch.equal(o, w[:, 0]) for o, w in zip(outs, want))
