"""Foreign-arena classification (proj_zoom on the volume entry points): what can be checked without a GPU -- the C ABI is declared,
exported and bound, the Python entry points take ``proj_zoom``, the shared shape helper rounds as scipy.ndimage.zoom does, and the
scikit-learn cases of tests/test_foreign_arena_gpu.py have the margins that test asserts."""
import ctypes
import inspect
import os
import re

import oracle_np as O
from conftest import ROOT

import foreign_arena_common as F

ENTRY_POINTS = ("rml_project_zoom", "rml_project_zoom_svm")


def test_header_library_and_binding_have_the_entry_points(built_lib, rml):
    from radar_ml_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "radarml.h")).read(), flags=re.S)
    lib = ctypes.CDLL(built_lib)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), "include/radarml.h does not declare %s" % name
        assert hasattr(lib, name), "libradarml_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # the argument counts of the declarations (out_shape is a host pointer, T an int, ld_feat an int64)
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define\s+RML_OPT_ZOOM_ROWS\s+(\d+)", txt).group(1)) == _lib.option_id("zoom_rows")


def test_volume_entry_points_take_proj_zoom(rml):
    for fn in (rml.process_volumes, rml.GpuSVC.decide_volumes, rml.GpuLinearClassifier.decide_volumes):
        params = inspect.signature(fn).parameters
        assert "proj_zoom" in params and params["proj_zoom"].default is None, fn
        assert list(params)[-1] == "proj_zoom", fn          # placed last: positional callers are unaffected


def test_shape_helper_gives_the_training_geometry(rml):
    z = rml.calc_proj_zoom(22, 31, 176, 20, 28, 160)
    assert rml.zoom_out_shapes(20, 28, 160, z) == ((22, 176), (31, 176), (22, 31))
    for name, (src, dst) in F.GRIDS.items():
        zo = F.zoom_of(name)
        assert rml.zoom_out_shapes(src[0], src[1], src[2], rml.ProjZoom(*zo)) == F.out_shapes(name), name
    # a scalar factor per plane zooms both axes, as scipy.ndimage.zoom takes it
    assert rml.zoom_out_shapes(10, 14, 40, rml.ProjZoom(1.1, 1.1, 1.1)) == ((11, 44), (15, 44), (11, 15))


def test_shape_helper_rounds_half_to_even(rml):
    # 10 * 1.25 = 12.5 and 10 * 1.35 = 13.5, both exact in binary: Python's round() gives 12 and 14 (scipy.ndimage.zoom's output
    # shape), round-half-up would give 13 and 14, truncation 12 and 13
    shapes = rml.zoom_out_shapes(10, 10, 10, rml.ProjZoom(xz=[1.25, 1.35], yz=[0.25, 0.45], xy=[1.05, 1.0]))
    assert 10 * 1.25 == 12.5 and 10 * 1.35 == 13.5 and 10 * 0.25 == 2.5 and 10 * 0.45 == 4.5 and 10 * 1.05 == 10.5
    assert shapes == ((12, 14), (2, 4), (10, 10))
    from scipy import ndimage
    import numpy as np
    assert ndimage.zoom(np.zeros((10, 10)), [1.25, 1.35]).shape == shapes[0]
    assert ndimage.zoom(np.zeros((10, 10)), [0.25, 0.45]).shape == shapes[1]


def test_unit_zoom_rule_is_that_of_process_samples(rml):
    from radar_ml_amd.common import is_unit_zoom
    one = rml.ProjZoom([1.0, 1.0], [1.0, 1.0], [1.0, 1.0])
    assert is_unit_zoom(None) and is_unit_zoom(one) and is_unit_zoom(rml.ProjZoom([1.0 + 1e-13, 1.0], [1.0, 1.0], [1.0, 1.0]))
    off = rml.ProjZoom([1.0, 1.0], [1.0, 1.0 + 1e-11], [1.0, 1.0])
    assert not is_unit_zoom(off)
    assert is_unit_zoom(off, rml.ProjMask(True, False, True))         # a plane that is masked out does not count


def test_sklearn_cases_have_the_margins_the_gpu_test_asserts():
    """tests/test_foreign_arena_gpu.py compares labels with scikit-learn's on every row: a 2e-7 row difference must not be able to
    decide one, so scikit-learn's own smallest |pair value| (score gap for the linear model) and top-2 probability gap are >= 1e-3."""
    for kind in ("svc", "sgd"):
        first, gap = F.sklearn_margins(kind)
        assert first >= F.MARGIN and gap >= F.MARGIN, (kind, first, gap)


def test_reference_rows_have_the_model_length():
    for name in F.GRIDS:
        n = 2
        rows = F.reference_rows(name, F.volumes(name, n), "max")
        assert rows.shape == (n, F.feature_len(name))
    assert F.feature_len("up") == 1364 and F.feature_len("walabot") == 10010
    z = F.zoom_of("walabot")
    assert list(z.xz) == list(O.calc_proj_zoom(22, 31, 176, 20, 28, 160).xz)
