"""No GPU: the float64 twins, bounds and cases of conv_train_common.py are fit to judge csrc/conv_train.hip, and the Python side of the
`convolutions="hip"` switch behaves on a machine without a device."""
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_train_common as T

CASES = T.cases()
SMALL = [c for c in CASES if c["N"] * c["Ho"] * c["Wo"] <= 600]
ids = lambda c: c["name"]


def _torch_reference(d):
    x = torch.from_numpy(d["X"]).permute(0, 3, 1, 2).requires_grad_(True)
    w = torch.from_numpy(d["W"]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    z = F.conv2d(x, w, None, stride=2)
    z.backward(torch.from_numpy(d["dZ"]).permute(0, 3, 1, 2))
    return (z.detach().permute(0, 2, 3, 1).numpy(), x.grad.permute(0, 2, 3, 1).numpy(), w.grad.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("c", SMALL, ids=ids)
def test_twins_equal_float64_conv2d_and_its_autograd(c):
    d = T.make(c)
    z, dx, dw = _torch_reference(d)
    for name, got, ref in (("forward", T.forward(d["X"], d["W"]), z), ("dgrad", T.dgrad(d["dZ"], d["W"]), dx),
                           ("wgrad", T.wgrad(d["X"], d["dZ"]), dw)):
        val, asum = got
        assert val.shape == ref.shape, name
        assert np.abs(val - ref).max() <= 1e-12 * max(1.0, asum.max()), name
        assert (asum >= np.abs(val) * (1 - 1e-12)).all(), name


def test_every_case_reaches_its_path():
    assert {c["path"] for c in CASES} == {"one", "row", "col", "tail", "mini", "big", "split"}
    for c in CASES:
        assert T.reaches(c), c["name"]
    for kind in T.KINDS:
        for pair in T.PAIRS:
            assert any(c["kind"] == kind and c["cin"] == pair[0] and c["sparse"] for c in CASES)
    assert T.wgrad_plan(T.SPLIT_PIXELS) == (3, 192)
    nc = importlib.import_module("radar_ml_amd.nn_common")
    for P in (1, 63, 64, 65, 255, 256, 257, 552, 4096, 256 * 128, 256 * 128 + 1, 1 << 20):
        assert nc.conv3s2_wgrad_plan(P) == T.wgrad_plan(P), P
        pieces, ln = T.wgrad_plan(P)
        assert ln % T.CHP == 0 and (pieces - 1) * ln < P <= pieces * ln and pieces <= T.MAX_PIECES
        assert nc.conv3s2_wgrad_chain(P, 128) == ln + pieces and nc.conv3s2_wgrad_chain(P, 64) == ln + 2 * pieces


@pytest.mark.parametrize("which,mutation", [(w, m) for w, ms in T.MUTATIONS.items() for m in ms])
def test_each_mutation_exceeds_its_bound_on_some_case(which, mutation):
    caught = []
    for c in SMALL:
        d = T.make(c)
        args = dict(forward=(d["X"], d["W"]), dgrad=(d["dZ"], d["W"]), wgrad=(d["X"], d["dZ"]))[which]
        fn = getattr(T, which)
        ref, asum = fn(*args)
        bad, _ = fn(*args, mutation=mutation)
        b = T.bound(ref, asum, T.chains(c)[which], c["kind"])
        if (np.abs(bad - ref) > b).any():
            caught.append(c["name"])
    print(which, mutation, "caught on", len(caught), "of", len(SMALL))
    assert caught


def test_conv3s2_on_cpu_is_conv2d_bit_for_bit():
    nc = importlib.import_module("radar_ml_amd.nn_common")
    torch.manual_seed(0)
    for dt, cin, cout in ((torch.float32, 128, 64), (torch.bfloat16, 64, 32), (torch.float32, 5, 7)):
        x = torch.randn(2, cin, 9, 7).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = (torch.randn(cout, cin, 3, 3) * 0.1).to(dt).requires_grad_(True)
        assert not nc.conv3s2_supported(x, w)
        a = nc.conv3s2(x, w)
        b = F.conv2d(x, w, None, stride=2)
        assert torch.equal(a, b)
        g = torch.randn_like(a)
        ga = torch.autograd.grad(a, (x, w), g)
        gb = torch.autograd.grad(b, (x, w), g)
        assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


def test_hip_model_on_cpu_runs_the_plain_layers():
    sgan = importlib.import_module("radar_ml_amd.sgan")
    torch.manual_seed(1)
    lib_model = sgan.Discriminator(((16, 16, 1),) * 3, 3)
    assert lib_model.conv_impl == "library"
    hip_model = copy.deepcopy(lib_model)
    hip_model.conv_impl = "hip"
    x = [torch.randn(4, 1, 16, 16) for _ in range(3)]
    for m in (lib_model, hip_model):
        m.drop.p = 0.0
        m.train()
    a, b = lib_model(*x), hip_model(*x)
    assert torch.equal(a, b)
    assert sgan.define_discriminator((16, 16, 1), (16, 16, 1), (16, 16, 1), device="cpu", convolutions="hip").conv_impl == "hip"
    assert sgan.define_discriminator((16, 16, 1), (16, 16, 1), (16, 16, 1), device="cpu").conv_impl == "library"
    with pytest.raises(ValueError):
        sgan.define_discriminator(device="cpu", convolutions="x")


def test_trainer_refuses_an_unknown_convolutions_value():
    sgan = importlib.import_module("radar_ml_amd.sgan")
    model = sgan.Discriminator(((16, 16, 1),) * 3, 3)
    with pytest.raises(ValueError):
        sgan.DiscriminatorTrainer(model, convolutions="x")
    assert model.conv_impl == "library"
    tr = sgan.DiscriminatorTrainer(model, convolutions="hip")
    assert model.conv_impl == "hip" and tr.model is model
    assert sgan.DiscriminatorTrainer(copy.deepcopy(model)).model.conv_impl == "library"


def test_header_and_signatures_carry_the_five_entry_points():
    _lib = importlib.import_module("radar_ml_amd._lib")
    names = {"rml_conv3s2_supported", "rml_conv3s2_workspace_bytes", "rml_conv3s2_forward", "rml_conv3s2_dgrad", "rml_conv3s2_wgrad"}
    assert names <= set(_lib.SIGNATURES)
    import os
    txt = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "radarml.h")).read()
    for n in names:
        assert n + "(" in txt, n
