"""No GPU: the float64 twins, bounds and cases of convt_train_common.py are fit to judge csrc/convt_train.hip, and the Python side of
the generator's `convolutions="hip"` switch behaves on a machine without a device."""
import copy
import ctypes
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convt_train_common as T

CASES = T.cases()
SMALL = [c for c in CASES if c["N"] * c["H"] * c["W"] <= 576]
ids = lambda c: c["name"]
_MADE = {}


def made(c):
    """the case's arrays and float64 twins, computed once and never written to"""
    if c["name"] not in _MADE:
        d = T.make(c)
        d["forward"], d["dgrad"], d["wgrad"] = T.forward(d["X"], d["W"]), T.dgrad(d["dZ"], d["W"]), T.wgrad(d["X"], d["dZ"])
        for v in d.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
        _MADE[c["name"]] = d
    return _MADE[c["name"]]


def _torch_reference(d):
    x = torch.tensor(d["X"]).permute(0, 3, 1, 2).requires_grad_(True)
    w = torch.tensor(d["W"]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)           # (ci, co, 4, 4)
    z = F.conv_transpose2d(x, w, None, stride=2, padding=1)
    z.backward(torch.tensor(d["dZ"]).permute(0, 3, 1, 2))
    return (z.detach().permute(0, 2, 3, 1).numpy(), x.grad.permute(0, 2, 3, 1).numpy(), w.grad.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("c", SMALL, ids=ids)
def test_twins_equal_float64_conv_transpose2d_and_its_autograd(c):
    d = made(c)
    z, dx, dw = _torch_reference(d)
    for name, ref in (("forward", z), ("dgrad", dx), ("wgrad", dw)):
        val, asum = d[name]
        assert val.shape == ref.shape, name
        assert np.abs(val - ref).max() <= 1e-12 * max(1.0, asum.max()), name
        assert (asum >= np.abs(val) * (1 - 1e-12)).all(), name


def test_forward_twin_equals_the_generator_twin():
    """the scatter form the generator's own float64 twin is written in (Keras kernel (ky, kx, co, ci))"""
    from sgan_gen_common import conv_transpose_scatter
    d = made(CASES[0])
    ref = conv_transpose_scatter(d["X"], d["W"].transpose(1, 2, 3, 0), 0.0)
    assert np.abs(ref - d["forward"][0]).max() <= 1e-12 * d["forward"][1].max()


def test_every_case_reaches_its_path():
    assert {c["path"] for c in CASES} == {"one", "seamx", "seamy", "three", "split", "big"}
    assert sorted((c["N"], c["H"], c["W"], c["sparse"]) for c in CASES if c["kind"] == "float16") == sorted(
        [(1, 8, 8, False), (3, 8, 16, False), (3, 8, 16, True), (2, 16, 8, False), (2, 24, 8, False), (1, 24, 24, False), (4, 32, 32, False)])
    for c in CASES:
        assert T.reaches(c), c["name"]
    for kind in T.KINDS:
        assert any(c["kind"] == kind and c["sparse"] for c in CASES)


def test_plan_mirror_equals_the_modules_constants():
    assert T.wgrad_plan(T.SPLIT_PIXELS) == (5, 128)
    nc = importlib.import_module("radar_ml_amd.nn_common")
    for P in (64, 128, 192, 384, 576, 4096, 8192, 8256, 64 * 128 * 2, 32 * 64 * 64, 96 * 64 * 64, 1 << 21):
        assert nc.convt4s2_wgrad_plan(P) == T.wgrad_plan(P), P
        pieces, ln = T.wgrad_plan(P)
        assert ln % T.CHP == 0 and (pieces - 1) * ln < P <= pieces * ln and pieces <= T.MAX_PIECES
        assert nc.convt4s2_wgrad_chain(P) == ln + pieces


@pytest.mark.parametrize("which", ("forward", "dgrad", "wgrad"))
@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_each_mutation_exceeds_its_bound_on_every_small_case(which, mutation):
    nc = importlib.import_module("radar_ml_amd.nn_common")
    missed = []
    for c in SMALL:
        d = made(c)
        args = dict(forward=(d["X"], d["W"]), dgrad=(d["dZ"], d["W"]), wgrad=(d["X"], d["dZ"]))[which]
        ref, asum = d[which]
        bad, _ = getattr(T, which)(*args, mutation=mutation)
        # the looser of the two weight-gradient bounds (the whole pixel count): what escapes it escapes the kernel's chain as well
        b = T.bound(ref, asum, max(T.chains(c)[which], T.chains(c, nc.convt4s2_wgrad_chain)[which]), c["kind"])
        if not (np.abs(bad - ref) > b).any():
            missed.append(c["name"])
    assert not missed, (which, mutation, missed)


def test_library_exports_the_entry_points_and_answers_on_the_host():
    _lib = importlib.import_module("radar_ml_amd._lib")
    names = ("rml_convt4s2_supported", "rml_convt4s2_workspace_bytes", "rml_convt4s2_forward", "rml_convt4s2_dgrad", "rml_convt4s2_wgrad")
    assert set(names) <= set(_lib.SIGNATURES)
    import os
    txt = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "radarml.h")).read()
    for n in names:
        assert n + "(" in txt, n
    for n in ("RML_CONVT4S2_FORWARD 0", "RML_CONVT4S2_DGRAD 1", "RML_CONVT4S2_WGRAD 2"):
        assert "#define " + n in txt, n
    build = importlib.import_module("radar_ml_amd.build")
    so = ctypes.CDLL(build.build())
    for n in names + ("rml_last_error",):
        assert hasattr(so, n), n
    sup = so.rml_convt4s2_supported
    sup.restype, sup.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    for args in ((128, 128, 8, 8), (128, 128, 8, 128), (128, 128, 128, 128), (128, 128, 24, 16)):
        assert sup(*args) == 1, args
    for args in ((128, 64, 8, 8), (64, 64, 8, 8), (128, 128, 4, 8), (128, 128, 12, 8), (128, 128, 8, 136), (128, 128, 0, 8), (128, 128, 8, -8)):
        assert sup(*args) == 0, args
    wsb = so.rml_convt4s2_workspace_bytes
    wsb.restype = ctypes.c_int64
    wsb.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int] * 5
    assert wsb(None, 2, 8, 8, 128, 128, 0) == wsb(None, 2, 8, 8, 128, 128, 1) == 16 * 128 * 128 * 2
    for P_n, h, w in ((1, 24, 24), (4, 32, 32), (96, 64, 64)):
        assert wsb(None, P_n, h, w, 128, 128, 2) == T.wgrad_plan(P_n * h * w)[0] * 16 * 128 * 128 * 4
    assert wsb(None, 2, 12, 8, 128, 128, 0) == 0 and wsb(None, 2, 8, 8, 128, 64, 2) == 0 and wsb(None, 2, 8, 8, 128, 128, 3) == 0


def test_convt4s2_on_cpu_is_conv_transpose2d_bit_for_bit():
    nc = importlib.import_module("radar_ml_amd.nn_common")
    torch.manual_seed(0)
    for dt, cin, cout, h, w in ((torch.float32, 128, 128, 8, 8), (torch.bfloat16, 128, 128, 8, 16), (torch.float32, 5, 7, 3, 6)):
        x = torch.randn(2, cin, h, w).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        k = (torch.randn(cin, cout, 4, 4) * 0.1).to(dt).requires_grad_(True)
        assert not nc.convt4s2_supported(x, k)
        a = nc.convt4s2(x, k)
        b = F.conv_transpose2d(x, k, None, stride=2, padding=1)
        assert a.shape == (2, cout, 2 * h, 2 * w) and torch.equal(a, b)
        g = torch.randn_like(a)
        ga = torch.autograd.grad(a, (x, k), g)
        gb = torch.autograd.grad(b, (x, k), g)
        assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


def test_hip_generator_on_cpu_runs_the_plain_layers():
    sgan = importlib.import_module("radar_ml_amd.sgan")
    torch.manual_seed(1)
    lib_model = sgan.Generator(latent_dim=100, channels=128, base=8, n_up=1)
    assert lib_model.conv_impl == "library"
    hip_model = copy.deepcopy(lib_model)
    hip_model.conv_impl = "hip"
    z = torch.randn(4, 100)
    outs = []
    for m in (lib_model, hip_model):
        m.train()
        imgs = m(z)
        grads = torch.autograd.grad(sum((o * o).sum() for o in imgs), [p for k, p in m.named_parameters() if not k.endswith("ups.0.bias")])
        outs.append((imgs, grads, {k: v.clone() for k, v in m.state_dict().items()}))
    for a, b in zip(outs[0][0] + list(outs[0][1]), outs[1][0] + list(outs[1][1])):
        assert torch.equal(a, b)
    for k, v in outs[0][2].items():
        assert torch.equal(v, outs[1][2][k]), k


def test_unknown_convolutions_values_are_refused_and_the_default_is_library():
    sgan = importlib.import_module("radar_ml_amd.sgan")
    with pytest.raises(ValueError):
        sgan.define_generator(device="cpu", convolutions="x")
    gen = sgan.Generator(latent_dim=100, channels=128, base=8, n_up=1)
    disc = sgan.Discriminator(((16, 16, 1),) * 3, 3)
    dt = sgan.DiscriminatorTrainer(disc)
    with pytest.raises(ValueError):
        sgan.GanTrainer(gen, dt, convolutions="x")
    assert gen.conv_impl == "library"
    assert sgan.GanTrainer(gen, dt).generator.conv_impl == "library"
    assert sgan.GanTrainer(gen, dt, convolutions="hip").generator.conv_impl == "hip"
    assert sgan.GanTrainer(gen, dt).generator.conv_impl == "hip"                  # None leaves the attribute
    assert sgan.GanTrainer(gen, dt, convolutions="library").generator.conv_impl == "library"
