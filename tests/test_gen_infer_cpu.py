"""The SGAN generator's fused inference chain, the parts that need no GPU: the BatchNorm fold and the packed layouts of
``rml_sgan_generate`` against a float64 NumPy twin that computes the transposed convolution by output phases (and mutations of the
twin that must NOT agree), the cache key of the packs, the unchanged default of ``Generator.predict``, the errors, the C ABI."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from gen_infer_common import (CHAIN_CASES, MUTATIONS, in_band, make_generator, make_latent, packs_numpy, plain_eval, twin_generate,
                              twin_packs)

NEW_SYMBOLS = ("rml_gen_up_supported", "rml_gen_up_forward", "rml_sgan_generate_workspace_bytes", "rml_sgan_generate")


@pytest.fixture(scope="module")
def sgan(rml):
    return importlib.import_module("radar_ml_amd.sgan")


@pytest.fixture(scope="module")
def small():
    """(float64 model, latent points, its plain eval images as (n, S, S) NumPy): Generator(5, 8, 8, 2), batch 3"""
    model = make_generator(5, 8, 8, 2, seed=1, dtype=torch.float64)
    z = make_latent(3, 5, seed=1, dtype=torch.float64)
    ref = [v[:, 0].numpy() for v in plain_eval(model, z)]
    return model, z, ref


def _err(got, ref):
    return max(float(np.abs(g - r).max()) for g, r in zip(got, ref))


def test_new_symbols_declared_and_bound(rml):
    """the four entry points are in the header, in the binding and in the library: on the parent commit this import fails"""
    from radar_ml_amd import _lib
    txt = open(os.path.join(ROOT, "include", "radarml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in include/radarml.h" % s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    for name in ("fold_generator", "generator_packs", "generate_dataset", "define_generator"):
        assert callable(getattr(rml, name))


def test_gen_up_supported_on_the_host(rml):
    from radar_ml_amd import _lib
    lib = _lib.load()
    for H, W, C, want in ((8, 8, 128, 1), (128, 128, 128, 1), (8, 24, 128, 1), (64, 16, 128, 1), (136, 8, 128, 0), (8, 136, 128, 0),
                          (4, 8, 128, 0), (8, 0, 128, 0), (12, 8, 128, 0), (8, 20, 128, 0), (8, 8, 64, 0), (8, 8, 8, 0), (-8, 8, 128, 0)):
        assert lib.rml_gen_up_supported(H, W, C) == want, (H, W, C)
    assert lib.rml_sgan_generate_workspace_bytes(2, 8, 4, 128) == 2 * (128 * 128 * 128 * 2 + 64 * 64 * 128 * 2)
    assert lib.rml_sgan_generate_workspace_bytes(2, 8, 1, 128) == 2 * (8 * 8 * 128 * 2 + 16 * 16 * 128 * 2)
    big = [lib.rml_sgan_generate_workspace_bytes(n, 8, 4, 128) for n in (1, 16, 100, 4096, 10 ** 6)]
    assert big == sorted(big) and big[-1] == big[-2] <= 128 << 20          # chunked: bounded, non-decreasing
    for base, n_up, C in ((8, 4, 8), (8, 6, 128), (4, 1, 128), (12, 1, 128), (8, -1, 128)):
        assert lib.rml_sgan_generate_workspace_bytes(2, base, n_up, C) == 0, (base, n_up, C)


def test_inputs_touch_every_border(small):
    """input and weights are non-zero on every border row and column, so a wrong tap or halo shows"""
    model, z, _ = small
    for br in model.branches:
        h = torch.relu(br.dense(z)).detach().reshape(-1, 8, 8, 8)
        for edge in (h[:, 0], h[:, -1], h[:, :, 0], h[:, :, -1]):
            assert float(edge.abs().sum()) > 0 and bool((edge.abs().amax(dim=-1) > 0).all())
        for up in br.ups:
            assert bool((up.weight != 0).all())


def test_fold_and_packs_against_the_twin(sgan, small):
    model, z, ref = small
    kw = model.keras_weights()
    mine = twin_packs(kw)
    prod = packs_numpy(sgan.generator_packs(model, torch.float64))
    assert sorted(prod) == sorted(mine)
    for k in mine:
        assert prod[k].shape == mine[k].shape, k
        assert float(np.abs(prod[k] - mine[k]).max()) <= 1e-12, k
    f = sgan.fold_generator(model)
    assert len(f) == 3 and len(f[0][1]) == 2 and tuple(f[0][1][0][0].shape) == (4, 4, 8, 8) and f[0][1][0][0].dtype == torch.float64
    assert tuple(f[0][0][0].shape) == (5, 8 * 8 * 8) and tuple(f[0][2][0].shape) == (7, 7, 8, 1)
    # the packed layouts through the phase arithmetic reproduce the plain eval model
    for packs in (prod, mine):
        got = twin_generate(z.numpy(), packs, 8)
        e = _err(got, ref)
        print("twin on the packed layouts against the plain float64 layers: %.3e" % e)
        assert got[0].shape == (3, 32, 32) and e <= 1e-12
    # the default packs are bfloat16 for the kernels, float32 for the rest
    pk = sgan.generator_packs(model.float())
    assert pk["up_wt"].dtype == torch.bfloat16 and tuple(pk["up_wt"].shape) == (3, 2, 4, 8, 32)
    assert all(pk[k].dtype == torch.float32 for k in ("dense_w", "dense_b", "up_bias", "out_w", "out_b"))


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutations_of_the_twin_disagree(small, mutation):
    model, z, ref = small
    got = twin_generate(z.numpy(), twin_packs(model.keras_weights(), mutation), 8, mutation)
    e = _err(got, ref)
    print("mutation %s: error %.3e" % (mutation, e))
    assert np.isfinite(e) and e > 1e-6


def test_pack_key(sgan):
    model = make_generator(5, 8, 8, 2, seed=2)
    z = make_latent(2, 5, seed=2)
    k0 = model.packs_key()
    p0 = sgan.generator_packs(model)
    model.predict(z)
    model.predict(z)
    assert model.packs_key() == k0 and sgan.generator_packs(model) is p0         # two inference calls: no change
    with torch.no_grad():
        model.branches[1].ups[0].weight.mul_(1.5)
    k1 = model.packs_key()
    assert k1 != k0
    p1 = sgan.generator_packs(model)
    assert p1 is not p0 and not torch.equal(p1["up_wt"], p0["up_wt"])
    model.train()
    model(z)                                                                    # training-mode forward: the moving statistics advance
    model.eval()
    assert model.packs_key() != k1
    p2 = sgan.generator_packs(model)
    assert p2 is not p1 and not torch.equal(p2["up_bias"], p1["up_bias"])
    with torch.no_grad():
        model.branches[2].bns[1].running_var.add_(0.25)                          # a buffer alone
    assert sgan.generator_packs(model) is not p2
    k3 = model.packs_key()
    model.set_keras_weights(model.keras_weights())
    assert model.packs_key() != k3


def test_predict_defaults_are_the_plain_eval_layers(sgan):
    model = make_generator(5, 8, 8, 2, seed=3)
    z = make_latent(4, 5, seed=3)
    want = plain_eval(model, z)
    got = model.predict(z.numpy())
    got_t = model.predict(z, return_numpy=False)
    for w, g, t in zip(want, got, got_t):
        assert g.shape == (4, 32, 32, 1) and g.dtype == np.float32
        assert np.array_equal(g, w.permute(0, 2, 3, 1).numpy()) and torch.equal(t, w)
    import inspect
    for fn, name in ((sgan.Generator.predict, "fused"), (sgan.generate_fake_samples, "fused"), (sgan.generated_samples, "fused"),
                     (sgan.train, "fused_generate")):
        assert inspect.signature(fn).parameters[name].default is False
    assert inspect.signature(sgan.generate_dataset).parameters["fused"].default is True
    rng_a, rng_b = np.random.default_rng(7), np.random.default_rng(7)
    xa, ya = sgan.generate_fake_samples(model, 5, 3, rng_a)
    z3 = sgan.generate_latent_points(5, 3, rng_b)
    assert np.array_equal(xa[0], model.predict(z3)[0])


def test_fused_on_a_cpu_model_raises(sgan):
    model = make_generator(5, 128, 8, 1, seed=4)
    z = make_latent(2, 5, seed=4)
    with pytest.raises(ValueError):
        model.predict(z, fused=True)
    with pytest.raises(ValueError):
        model.forward_fused(z)
    with pytest.raises(ValueError):
        sgan.generate_fake_samples(model, 5, 2, np.random.default_rng(0), fused=True)
    with pytest.raises(ValueError):
        sgan.generate_dataset(model, 2, latent_dim=5, rng=np.random.default_rng(0))
    assert len(sgan.generate_dataset(model, 0, latent_dim=5)) == 0


@pytest.mark.parametrize("case", [c for c in CHAIN_CASES if c[4] <= 3])
def test_images_are_neither_flat_nor_saturated(case):
    """the condition on the test model: at least half the pixels of every image of every chain case have |v| in [0.05, 0.95] in the
    plain float32 model (the batch-9 and batch-5 cases share their model family with the smaller batches checked here)"""
    latent_dim, channels, base, n_up, B, seed = case
    model = make_generator(latent_dim, channels, base, n_up, seed)
    frac = in_band(plain_eval(model, make_latent(B, latent_dim, seed)))
    print("case %s: %.3f of the pixels in the band" % (case, frac))
    assert frac >= 0.5
