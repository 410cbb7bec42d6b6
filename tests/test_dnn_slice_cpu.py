"""CNN / SGAN classification of target slices (rml_dnn_preprocess_slices, predict_volumes(mode="slice", ijk=(B,T,3))): what can be
checked without a GPU -- the C ABI is declared, exported and bound, the row <-> (frame, target) arithmetic of the margin guard's
callback, the Python surface, and that the test targets cover what tests/test_dnn_slice_gpu.py says they cover."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from conftest import ROOT

import dnn_slice_common as S

ENTRY = "rml_dnn_preprocess_slices"


def test_header_library_and_binding_have_the_entry_point(built_lib, rml):
    from radar_ml_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "radarml.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, txt), "include/radarml.h does not declare %s" % ENTRY
    assert hasattr(ctypes.CDLL(built_lib), ENTRY), "libradarml_hip.so does not export %s" % ENTRY
    assert ENTRY in _lib.SIGNATURES
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % ENTRY, txt, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[ENTRY][1]) == 15


def test_row_to_frame_and_target(rml):
    from radar_ml_amd.nn_common import slice_row_targets
    # T = 3: row b * 3 + t; unsorted rows, a repeat, the last row of a 4-frame batch
    rows = [7, 0, 2, 11, 3, 7]
    f, t = slice_row_targets(rows, 3)
    assert f.tolist() == [2, 0, 0, 3, 1, 2] and t.tolist() == [1, 0, 2, 2, 0, 1]
    # T = 1: a row is its frame
    f, t = slice_row_targets(np.array([5, 1, 4]), 1)
    assert f.tolist() == [5, 1, 4] and t.tolist() == [0, 0, 0]
    # torch index tensors (what the guard hands over) keep their kind and dtype
    f, t = slice_row_targets(torch.tensor([9, 4, 5], dtype=torch.int64), 4)
    assert isinstance(f, torch.Tensor) and f.dtype == torch.int64 and f.tolist() == [2, 1, 1] and t.tolist() == [1, 0, 1]
    f, t = slice_row_targets(np.zeros((0,), dtype=np.int64), 2)
    assert f.shape == (0,) and t.shape == (0,)
    # and back: b * T + t
    rows = np.array([13, 2, 8])
    f, t = slice_row_targets(rows, 5)
    assert (f * 5 + t).tolist() == rows.tolist()
    with pytest.raises(ValueError):
        slice_row_targets([0], 0)
    with pytest.raises(TypeError):
        slice_row_targets([0.5], 2)


def test_predict_volumes_takes_targets_and_has_no_cpu_path(rml):
    from radar_ml_amd import dnn, sgan, predict
    for fn in (dnn.Classifier.predict_volumes, sgan.Discriminator.predict_volumes, dnn.Classifier.rescore_exact):
        assert "ijk" in inspect.signature(fn).parameters, fn
    for fn in (dnn.Classifier.predict_volumes, sgan.Discriminator.predict_volumes):
        p = inspect.signature(fn).parameters
        assert p["ijk"].default is None and p["num_targets"].default == 1 and p["return_ijk"].default is False, fn
    p = inspect.signature(predict.classify_targets).parameters
    assert list(p) == ["model", "class_names", "volumes", "ijk", "num_targets", "min_proba"] and p["min_proba"].default == 0.7
    model = dnn.define_classifier(device="cpu").eval()
    vol = np.zeros((2, 5, 7, 16), dtype=np.uint8)
    ijk = np.zeros((2, 3, 3), dtype=np.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.predict_volumes(vol, mode="slice", ijk=ijk)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.predict_volumes(vol, mode="slice", ijk=ijk[:, 0])
    with pytest.raises(ValueError, match="one row"):
        model.predict_volumes(vol, mode="slice", ijk=ijk[:1])


def test_classify_targets_names_through_classify_batch(rml):
    """classify_targets on a stand-in model: 'Unknown' below min_proba, the class name at or above it, one (name, proba) per target."""
    from radar_ml_amd import predict

    class Model:
        def predict_volumes(self, volumes, mode, ijk, num_targets):
            self.seen = (mode, ijk, num_targets)
            return torch.tensor([[0.1, 0.8, 0.1], [0.4, 0.35, 0.25], [0.7, 0.2, 0.1]])
    m = Model()
    names, proba = predict.classify_targets(m, ["cat", "dog", "person"], np.zeros((1, 2, 2, 16)), ijk=None, num_targets=3)
    assert names == ["dog", "Unknown", "cat"] and np.allclose(proba, [0.8, 0.4, 0.7])
    assert m.seen == ("slice", None, 3)


def test_targets_cover_the_edges():
    for grid, rescale in S.GRIDS:
        t = S.targets(grid).astype(np.int64)
        size = np.array(grid)
        assert t.shape == (S.B, 3, 3) and ((t >= -size) & (t < size)).all()
        flat = t.reshape(-1, 3)
        for ax in range(3):
            assert 0 in flat[:, ax] and grid[ax] - 1 in flat[:, ax] and -grid[ax] in flat[:, ax]
        assert (flat < 0).any()
        assert any((t[b, u] == t[b, w]).all() for b in range(S.B) for u in range(3) for w in range(u + 1, 3))
        assert any((t[b, u, :2] == t[b, w, :2]).all() and t[b, u, 2] != t[b, w, 2] for b in range(S.B) for u in range(3) for w in range(u + 1, 3))
        v = S.volumes(grid, "f32_off")
        assert (v[1] != np.round(v[1])).any() and v[1].max() > 255 and (v[0] == np.round(v[0])).all() and v[0].max() <= 255
        xz, yz, xy = S.numpy_planes(v, S.targets(grid))
        assert xz.shape == (9,) + (grid[0], grid[2]) and yz.shape == (9,) + (grid[1], grid[2]) and xy.shape == (9,) + (grid[0], grid[1])
        assert max(p[3].max() for p in (xz, yz, xy)) > 255          # row 1 * 3 + 0 sees the value above 255
