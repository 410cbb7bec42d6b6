"""SGAN classifier inference, the parts that need no GPU: the BatchNorm folding against the model in float64, the host-only shape rule
of the fused trunk, and the version-counter key of the folded weight packs."""
import importlib

import pytest
import torch

from sgan_infer_common import folded_eval, make_model, make_planes, plain_eval


@pytest.fixture(scope="module")
def sgan(rml):
    return importlib.import_module("radar_ml_amd.sgan")


@pytest.mark.parametrize("C", [3, 5])
@pytest.mark.parametrize("H,W", [(16, 16), (16, 40)])
def test_folded_layers_equal_eval_model_in_float64(sgan, H, W, C):
    """fold_batchnorm: the folded convolutions and dense layers + LeakyReLU, applied with plain F.conv2d / F.linear in float64, are the
    inference-mode model in float64 to 1e-12 (features and class scores); folded_packs holds those tensors in the kernels' layouts:
    k = (ky * 3 + kx) * Cin + cin, fc2 transposed, bf16 where the matrix cores read them."""
    model = make_model(H, W, C, seed=H + W + C, dtype=torch.float64)
    xs = make_planes(3, H, W, seed=C, dtype=torch.float64)
    fv_ref, p_ref = plain_eval(model, xs)
    with torch.no_grad():
        lg_ref = model(*[x.unsqueeze(1) for x in xs])
    folded = sgan.fold_batchnorm(model)
    fv, lg = folded_eval(folded, xs)
    assert fv.dtype == torch.float64 and fv.shape == (3, (H // 8) * (W // 8) * 96)
    assert float((fv - fv_ref).abs().max()) <= 1e-12
    assert float((lg - lg_ref).abs().max()) <= 1e-12
    assert float((torch.softmax(lg, dim=-1) - p_ref).abs().max()) <= 1e-12
    pk = sgan.folded_packs(model)
    assert pk["w1"].shape == (3, 128, 9) and pk["w1"].dtype == torch.float32 and pk["b1"].shape == (3, 128)
    assert pk["w2t"].shape == (3, 64, 1152) and pk["w2t"].dtype == torch.bfloat16 and pk["b2"].shape == (3, 64)
    assert pk["w3t"].shape == (3, 32, 576) and pk["w3t"].dtype == torch.bfloat16 and pk["b3"].shape == (3, 32)
    for br in range(3):
        (w1, b1), (w2, b2), (w3, b3) = folded["conv"][br]
        assert torch.equal(pk["w1"][br].reshape(128, 3, 3), w1[:, 0].float())
        assert torch.equal(pk["w2t"][br].reshape(64, 3, 3, 128).permute(0, 3, 1, 2), w2.to(torch.bfloat16))
        assert torch.equal(pk["w3t"][br].reshape(32, 3, 3, 64).permute(0, 3, 1, 2), w3.to(torch.bfloat16))
        assert torch.equal(pk["b1"][br], b1.float()) and torch.equal(pk["b2"][br], b2.float()) and torch.equal(pk["b3"][br], b3.float())
    assert torch.equal(pk["fc1_w"], folded["fc"][0][0].to(torch.bfloat16)) and torch.equal(pk["fc2_wt"], folded["fc"][1][0].float().t())
    assert torch.equal(pk["fc3_w"], folded["fc"][2][0].float()) and pk["slope"] == 0.2


def test_trunk_supported_rule_and_workspace(rml):
    """rml_sgan_trunk_supported (host only): H and W multiples of 8, W <= 128; the workspace size is monotone in B and 0 for planes
    the trunk does not take."""
    from radar_ml_amd import _lib
    lib = _lib.load()
    for hw in ((8, 8), (16, 40), (128, 128)):
        assert lib.rml_sgan_trunk_supported(*hw) == 1, hw
    for hw in ((12, 16), (128, 136), (0, 8), (16, 12), (-8, 8), (8, 0)):
        assert lib.rml_sgan_trunk_supported(*hw) == 0, hw
        assert lib.rml_sgan_trunk_workspace_bytes(4, *hw) == 0
    for H, W in ((8, 8), (16, 40), (128, 128)):
        sizes = [lib.rml_sgan_trunk_workspace_bytes(B, H, W) for B in (0, 1, 2, 3, 9, 33, 4096)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert all(s % 16 == 0 for s in sizes)
    assert lib.rml_sgan_trunk_workspace_bytes(-1, 8, 8) == 0


def test_folded_packs_are_rebuilt_after_a_batchnorm_buffer_changes(sgan):
    """The pack cache keys on the version counters of every parameter AND every BatchNorm buffer: a pack built before an in-place
    change of a moving mean is not handed out after it; an unchanged model gets the cached pack."""
    model = make_model(16, 16, 3, seed=9)
    p1 = model.folded_packs()
    assert model.folded_packs() is p1
    bn = model.branches[1][1]
    with torch.no_grad():
        bn.running_mean.add_(0.25)
    p2 = model.folded_packs()
    assert p2 is not p1
    assert not torch.equal(p2["b1"][1], p1["b1"][1]) and torch.equal(p2["b1"][0], p1["b1"][0])
    assert torch.equal(p2["b1"], sgan.folded_packs(model)["b1"])
    with torch.no_grad():
        model.fc2.weight.mul_(1.5)
    p3 = model.folded_packs()
    assert p3 is not p2 and not torch.equal(p3["fc2_wt"], p2["fc2_wt"])
    with torch.no_grad():
        model.bn1.num_batches_tracked += 1          # what a training-mode forward does to every BatchNorm
    assert model.folded_packs() is not p3
