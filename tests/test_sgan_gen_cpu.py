"""SGAN generator, GAN step and fake-sample helpers on the CPU (float32 / float64 plain layers): sizes, the NumPy twin, the
reference's define_gan freeze semantics, the data product's pickle."""
import copy
import importlib

import numpy as np
import pytest
import torch

from sgan_gen_common import random_keras_weights, twin_branch


@pytest.fixture(scope="module")
def sgan(rml):
    return importlib.import_module("radar_ml_amd.sgan")


def test_generator_sizes_and_predict(sgan):
    torch.manual_seed(0)
    g = sgan.define_generator(device="cpu")
    assert sum(p.numel() for p in g.parameters() if p.requires_grad) == 5651331
    stats = sum(b.numel() for k, b in g.named_buffers() if "running_" in k)
    assert sum(p.numel() for p in g.parameters()) + stats == 5654403
    out = g.predict(np.random.default_rng(0).standard_normal((1, 100)))
    assert len(out) == 3
    for o in out:
        assert o.shape == (1, 128, 128, 1) and o.dtype == np.float32 and float(np.abs(o).max()) <= 1.0
    dev = g.predict(np.zeros((1, 100)), return_numpy=False)
    assert all(tuple(t.shape) == (1, 1, 128, 128) and t.dtype == torch.float32 for t in dev)


def test_generator_matches_numpy_twin_and_keras_round_trip(sgan):
    rng = np.random.default_rng(3)
    g = sgan.Generator(latent_dim=5, channels=8, base=8, n_up=2).double()
    w = random_keras_weights(g, rng)
    g.set_keras_weights(w)
    back = g.keras_weights()
    flat_a, flat_b = sgan._flatten_weights(w), sgan._flatten_weights(back)
    assert flat_a.keys() == flat_b.keys() and len(flat_a) == 3 * (2 + 2 * 6 + 2)
    for k in flat_a:
        assert np.array_equal(np.asarray(flat_a[k], np.float64), flat_b[k]), k
    z = rng.standard_normal((3, 5))
    g.eval()
    with torch.no_grad():
        ev = g(torch.from_numpy(z))
    g.train()
    with torch.no_grad():
        tr = g(torch.from_numpy(z))
    for b in range(3):
        for out, training in ((ev[b], False), (tr[b], True)):
            ref = twin_branch(z, w[b], 8, training)
            assert tuple(out.shape) == (3, 1, 32, 32)
            err = float(np.abs(out.permute(0, 2, 3, 1).numpy() - ref).max())
            assert err <= 1e-10, (b, training, err)
    # the training forward tracked the statistics of convT(x) + bias, although the bias is not added in front of the batch norm
    g2 = sgan.Generator(latent_dim=5, channels=8, base=8, n_up=2).double()
    g2.set_keras_weights(w)
    g2.train()
    br, br2 = g.branches[0], g2.branches[0]
    with torch.no_grad():
        h = torch.relu(br2.dense(torch.from_numpy(z))).reshape(3, 8, 8, 8).permute(0, 3, 1, 2)
        br2.bns[0](br2.ups[0](h))
    assert torch.allclose(br.bns[0].running_mean, br2.bns[0].running_mean, rtol=0, atol=1e-12)
    assert torch.allclose(br.bns[0].running_var, br2.bns[0].running_var, rtol=0, atol=1e-12)


def _small_gan(sgan, seed=1):
    torch.manual_seed(seed)
    g = sgan.Generator(latent_dim=6, channels=8, base=8, n_up=1)
    d = sgan.Discriminator(((16, 16, 1),) * 3, 3)
    dt = sgan.DiscriminatorTrainer(d, ddp=False)
    return g, d, dt, sgan.GanTrainer(g, dt)


def _bn_names(model):
    return {n + "." + s for n, m in model.named_modules() if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)) for s in ("weight", "bias")}


def test_gan_step_trains_generator_and_discriminator_batchnorm_only(sgan):
    g, d, dt, gan = _small_gan(sgan)
    rng = np.random.default_rng(2)
    x = [rng.uniform(-1, 1, (4, 16, 16, 1)).astype(np.float32) for _ in range(3)]
    dt.train_on_batch_c(x, rng.integers(0, 3, 4))           # the discriminator's optimizers have a state to keep
    dt.train_on_batch_d(x, np.full((4, 1), 0.9))
    d0, g0 = copy.deepcopy(d.state_dict()), copy.deepcopy(g.state_dict())
    opt0 = [copy.deepcopy(o.state_dict()) for o in (dt.opt_c, dt.opt_d)]
    lr = 2e-4
    z = sgan.generate_latent_points(6, 4, rng)
    loss = gan.train_on_batch_g(z, sgan.smooth_positive_labels(np.ones((4, 1)), rng))
    assert np.isfinite(loss)
    bn = _bn_names(d)
    assert len(bn) == 2 * (9 + 2)
    for k, v in d.state_dict().items():
        if k in bn:
            assert not torch.equal(v, d0[k]), k
            assert float((v - d0[k]).abs().max()) <= lr * (1 + 1e-3), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(d0[k]) + 1, k
        elif "running_" in k:
            assert not torch.equal(v, d0[k]), k
        else:
            assert torch.equal(v, d0[k]), k                 # every Conv / Linear weight and bias: bit for bit
    for k, v in g.state_dict().items():
        if ".ups." in k and k.endswith(".bias"):
            assert torch.equal(v, g0[k]) and float(v.abs().max()) == 0.0, k     # gradient exactly zero: stays exactly 0
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(g0[k]) + 1, k
        elif "running_" in k:
            assert not torch.equal(v, g0[k]), k
        else:
            assert not torch.equal(v, g0[k]), k
            assert float((v - g0[k]).abs().max()) <= lr * (1 + 1e-3), k
    for o, s0 in zip((dt.opt_c, dt.opt_d), opt0):
        s1 = o.state_dict()
        assert s1["state"].keys() == s0["state"].keys()
        for i in s0["state"]:
            for name, t in s0["state"][i].items():
                assert torch.equal(torch.as_tensor(t), torch.as_tensor(s1["state"][i][name])), (i, name)
    # the freeze does not leak out of the step: the next d update trains the convolutions again
    d1 = copy.deepcopy(d.state_dict())
    dt.train_on_batch_d(x, np.full((4, 1), 0.9))
    moved = [k for k, v in d.state_dict().items() if k.endswith("conv.weight") and not torch.equal(v, d1[k])]
    assert len(moved) == 9


def test_gan_step_leaves_grad_fields_alone(sgan):
    g, d, dt, gan = _small_gan(sgan, seed=4)
    rng = np.random.default_rng(5)
    x = [rng.uniform(-1, 1, (4, 16, 16, 1)).astype(np.float32) for _ in range(3)]
    dt.train_on_batch_d(x, np.full((4, 1), 0.9))
    before = {k: (None if p.grad is None else p.grad.clone()) for k, p in d.named_parameters()}
    ids = {k: id(p.grad) for k, p in d.named_parameters()}
    gan.train_on_batch_g(sgan.generate_latent_points(6, 4, rng), np.full((4, 1), 0.9))
    for k, p in d.named_parameters():
        assert id(p.grad) == ids[k], k
        assert (p.grad is None) == (before[k] is None) and (p.grad is None or torch.equal(p.grad, before[k])), k
    assert all(p.grad is None for p in g.parameters())


def test_gan_loss_falls_on_fixed_latent_points(sgan):
    g, d, dt, gan = _small_gan(sgan, seed=7)
    d.drop.p = 0.0
    rng = np.random.default_rng(8)
    z = sgan.generate_latent_points(6, 4, rng)
    y = np.full((4, 1), 0.9)
    losses = [gan.train_on_batch_g(z, y) for _ in range(30)]
    assert losses[-1] < losses[0], losses


def test_gan_trainer_refuses_data_parallel(sgan, monkeypatch):
    import torch.distributed as dist
    g, d, dt, gan = _small_gan(sgan)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError):
        sgan.GanTrainer(g, dt)


def test_fake_samples_and_generated_pickle(sgan, tmp_path):
    rml = importlib.import_module("radar_ml_amd")
    datasets = importlib.import_module("radar_ml_amd.datasets")
    torch.manual_seed(0)
    g = sgan.Generator(latent_dim=6, channels=8, base=8, n_up=1)
    rng = np.random.default_rng(9)
    imgs, y = sgan.generate_fake_samples(g, 6, 5, rng)
    assert len(imgs) == 3 and all(i.shape == (5, 16, 16, 1) and i.dtype == np.float32 for i in imgs)
    assert y.shape == (5, 1) and float(y.min()) >= 0.0 and float(y.max()) < 0.3
    z = sgan.generate_latent_points(6, 7, rng)
    assert z.shape == (7, 6)
    yp = sgan.smooth_positive_labels(np.ones((64, 1)), rng)
    assert float(yp.min()) >= 0.7 and float(yp.max()) < 1.2
    samples = [(rng.uniform(0, 255, (22, 176)).astype(np.float32), rng.uniform(0, 255, (31, 176)).astype(np.float32),
                rng.uniform(0, 255, (22, 31)).astype(np.float32)) for _ in range(4)]
    path = str(tmp_path / "generated_data_0001.pickle")
    assert sgan.save_generated(path, samples) == 4
    xz, yz, xy, labels = datasets.load_dataset(path)
    assert labels == ["generated_data"] * 4
    assert xz.shape == (4, 22, 176) and yz.shape == (4, 31, 176) and xy.shape == (4, 22, 31)
    for i, s in enumerate(samples):
        assert np.array_equal(xz[i], s[0]) and np.array_equal(yz[i], s[1]) and np.array_equal(xy[i], s[2])
    assert (sgan.XZ_SIZE, sgan.YZ_SIZE, sgan.XY_SIZE) == ((176, 22), (176, 31), (31, 22))
    assert rml.RADAR_MAX == 255.0


def test_conv7_binding_and_option_are_declared(rml):
    import os
    import re
    from conftest import ROOT
    from radar_ml_amd import _lib
    txt = open(os.path.join(ROOT, "include", "radarml.h")).read()
    for name in ("rml_conv7_tanh_supported", "rml_conv7_workspace_floats", "rml_conv7_tanh_forward", "rml_conv7_tanh_backward"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, txt)
    assert int(re.search(r"#define\s+RML_OPT_CONV7\s+(\d+)", txt).group(1)) == _lib.option_id("conv7")
    lib = _lib.load()
    assert lib.rml_conv7_tanh_supported(128, 128, 128) == 1 and lib.rml_conv7_tanh_supported(1, 256, 128) == 1
    assert lib.rml_conv7_tanh_supported(257, 8, 128) == 0 and lib.rml_conv7_tanh_supported(8, 8, 64) == 0
    assert lib.rml_conv7_tanh_supported(0, 8, 128) == 0
