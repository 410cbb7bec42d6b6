"""The SGAN classifier's margin guard, the parts that need no GPU: the near-tie fixture's conditions (from the float64 reference alone),
the float64 route of Discriminator.forward_exact against the .double() model, MarginGuard's stage thresholds as a constructor argument,
the public signatures, and the four new entry points in the header and the built library."""
import copy
import ctypes
import importlib
import inspect
import os
import re

import pytest
import torch

import sgan_guard_common as G
from conftest import ROOT
from dnn_guard_common import host_ops
from sgan_infer_common import make_model, make_planes, plain_eval

NEW_SYMBOLS = ("rml_sgan_trunk_x3_supported", "rml_sgan_trunk_x3_workspace_bytes", "rml_sgan_trunk_x3", "rml_dense_tail_lrelu_f32")


@pytest.mark.parametrize("spec", [G.SMALL, G.LARGE], ids=["16x16", "128x128"])
def test_fixture_conditions(rml, spec):
    """every float64 gap >= 1e-9, a row in each decade from 1e-6 to 1e-2, at least a third of the rows decided (gap > 0.2)"""
    fx = G.fixture(*spec)
    n = G.check_fixture(fx)
    assert n == spec[4] + spec[5] and tuple(fx[1][0].shape) == (n, spec[0], spec[1])
    print("fixture %dx%d: %d rows, float64 gaps %s" % (spec[0], spec[1], n, ", ".join("%.2e" % g for g in sorted(fx[3].tolist()))))


@pytest.mark.parametrize("H,W", [(8, 8), (16, 40), (40, 16)])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_float64_route_is_the_double_model(rml, C, H, W):
    """forward_exact(..., "float64") on the CPU (folded BatchNorm, im2col + matmul) against the .double() model's plain layers: <= 1e-12;
    the same result with model.train() set (inference mode holds whatever self.training says)"""
    model = make_model(H, W, C, seed=70 + C)
    xs = make_planes(5, H, W, seed=71)
    want = plain_eval(copy.deepcopy(model).double(), xs)[1]
    got = model.forward_exact(*xs, precision="float64")
    assert got.dtype == torch.float64 and got.shape == (5, C)
    err = float((got - want).abs().max())
    print("float64 route %dx%d C=%d: max |dp| = %.2e" % (H, W, C, err))
    assert err <= 1e-12
    model.train()
    try:
        again = model.forward_exact(*[x.unsqueeze(1) for x in xs], precision="float64")
        p32 = model.forward_exact(*xs, precision="float32")
    finally:
        model.eval()
    assert torch.equal(again, got)
    assert p32.dtype == torch.float32 and float((p32.double() - want).abs().max()) < 1e-4
    with pytest.raises(ValueError):
        model.forward_exact(*xs, precision="bf16")


def test_margin_guard_takes_its_stage_thresholds(rml):
    """MarginGuard(stages=...): the thresholds handed to GuardOps.apply are the custom ones; default construction gives STAGES"""
    dg = importlib.import_module("radar_ml_amd.dnn_guard")
    sgan = importlib.import_module("radar_ml_amd.sgan")
    assert dg.MarginGuard().stages == dg.STAGES
    assert inspect.signature(dg.MarginGuard.__init__).parameters["stages"].default is dg.STAGES
    mine = (dg.Stage("x3", 3e-3, True, "rescored", "observed_error"), dg.Stage("x6", 7e-4, False, "rescored_x6", "observed_error_x3"))
    exact = torch.tensor([[0.5002, 0.4998], [0.9, 0.1], [0.501, 0.499], [0.2, 0.8]], dtype=torch.float64)
    proba = exact.float().clone()
    proba[0] = torch.tensor([0.499, 0.501])
    ops = host_ops()
    w = torch.zeros(1)
    out = dg.MarginGuard(stages=mine).run(proba, 1e-2, lambda rows, prec: exact[rows].to(torch.float64 if prec == "float64" else torch.float32), ops, [w])
    applied = [c for c in ops.calls if c[0] == "apply"]
    assert [c[2] for c in applied] == [3e-3, 7e-4] and [c[3] for c in applied] == [True, False]
    assert applied[0][1] == [0, 2] and applied[1][1] == [0, 2] and torch.equal(out.argmax(dim=1), exact.argmax(dim=1))
    # the default cascade on the same table
    ops = host_ops()
    dg.MarginGuard().run(exact.float().clone(), 1e-2, lambda rows, prec: exact[rows].float(), ops, [w])
    assert [c[2] for c in ops.calls if c[0] == "apply"] == [dg.LABEL_GUARD_X3]
    # a float64 gap below float32's resolution: the float32 table would hold a tie (argmax 0); the float64 label (1) stays on top
    fine = torch.tensor([[0.5 - 1e-9, 0.5 + 1e-9], [0.7, 0.3]], dtype=torch.float64)
    assert int(fine.float().argmax(dim=1)[0]) == 0
    out = dg.MarginGuard().run(fine.float().clone(), 1e-2, lambda rows, prec: fine[rows].to(torch.float64 if prec == "float64" else torch.float32),
                               host_ops(), [w])
    assert out.dtype == torch.float32 and out.argmax(dim=1).tolist() == [1, 0] and float((out.double() - fine).abs().max()) < 1e-7
    # the SGAN classifier passes its own
    m = sgan.Discriminator(((8, 8, 1),) * 3, 2)
    assert [st.close for st in m._margin.stages] == [sgan.LABEL_GUARD_X3, sgan.LABEL_GUARD_X6] and m.last_guard is None


def test_signatures(rml):
    sgan = importlib.import_module("radar_ml_amd.sgan")
    D = sgan.Discriminator
    sig = inspect.signature(D.predict_volumes).parameters
    assert sig["label_guard"].default is None
    # the parent's parameters, in the parent's order, in front of the new one
    assert list(sig)[:11] == ["self", "volumes", "rescale", "mode", "ijk", "batch_size", "exact_resize", "return_numpy", "num_targets", "return_ijk",
                              "label_guard"]
    assert inspect.signature(D.forward_guarded).parameters["label_guard"].default == sgan.LABEL_GUARD
    assert inspect.signature(D.features_x3).parameters["parts"].default == 2
    assert list(inspect.signature(D.rescore_exact).parameters) == ["self", "volumes", "rescale", "mode", "precision", "rows", "ijk"]
    assert 0 < sgan.LABEL_GUARD_X6 <= sgan.LABEL_GUARD_X3 < sgan.LABEL_GUARD < 1


def test_header_and_library_export_the_new_entry_points(built_lib):
    txt = open(os.path.join(ROOT, "include", "radarml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(rml_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(built_lib)
    for s in NEW_SYMBOLS:
        assert s in declared, "include/radarml.h does not declare %s" % s
        assert hasattr(lib, s), "libradarml_hip.so does not export %s" % s
    # host-side answers (no device): 128 x 128 and the test sizes are taken, 12 x 16 is not; the workspace grows with the batch
    lib.rml_sgan_trunk_x3_workspace_bytes.restype = ctypes.c_int64
    lib.rml_sgan_trunk_x3_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    for hw in ((128, 128), (8, 8), (16, 16), (16, 40), (40, 16)):
        assert lib.rml_sgan_trunk_x3_supported(*hw) == 1
    assert lib.rml_sgan_trunk_x3_supported(12, 16) == 0 and lib.rml_sgan_trunk_x3_supported(16, 0) == 0
    assert lib.rml_sgan_trunk_x3_workspace_bytes(2, 12, 16) == 0
    w1, w2 = lib.rml_sgan_trunk_x3_workspace_bytes(1, 128, 128), lib.rml_sgan_trunk_x3_workspace_bytes(2, 128, 128)
    assert w2 - w1 == 3 * 32 * 32 * 64 * 4 and w1 > w2 - w1
