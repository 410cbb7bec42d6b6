"""radar-ml hot path on MI355X (gfx950): batched 3-D radar volume -> (xz, yz, xy) projections ->
feature rows -> RBF-SVM / linear decision -> labels, behind the reference's own call surface
(``common.process_samples`` / ``clf.predict`` / ``model.predict``).

Host code is Python and mirrors goruck/radar-ml's interface for this path; the work is done by
hand-written HIP kernels in ``libradarml_hip.so`` (C ABI in ``include/radarml.h``, bound with
ctypes in ``_lib.py``).  There is no CPU fallback.
"""
from . import _lib
from ._lib import RadarMLError
from .common import (ProjMask, ProjZoom, DerivedTarget, RADAR_MAX, RADAR_MIN,
                     cartesian_to_spherical, spherical_to_cartesian, calculate_matrix_indices,
                     process_samples, process_volumes, project, derive_targets, feature_len, zoom_out_shapes)
from .svm import GpuSVC, GpuCalibratedClassifier, GpuLinearClassifier, KernelMatrix, from_sklearn
from .predict import classifier, classify_batch, calc_proj_zoom
from .synth import synth_volumes
from .augment import DataGenerator, augment_planes, rotation_params
from .train import (GridSearchSVC, find_best_svm_estimator, fit_svc, GridSearchSGD, find_best_sgd_svm_estimator, fit_sgd,
                    partial_fit_sgd, partial_fit_sgd_steps, balance_classes, balance_indices, sgd_fit, svc_fit, calibrate_prefit,
                    evaluate_model, ProjMaskSearchSVC, find_best_proj_mask_svm_estimator, svc_fit_masks)

__all__ = [
    "RadarMLError", "ProjMask", "ProjZoom", "DerivedTarget", "RADAR_MAX", "RADAR_MIN",
    "cartesian_to_spherical", "spherical_to_cartesian", "calculate_matrix_indices",
    "process_samples", "process_volumes", "project", "derive_targets", "feature_len", "zoom_out_shapes",
    "GpuSVC", "GpuCalibratedClassifier", "GpuLinearClassifier", "KernelMatrix", "from_sklearn",
    "classifier", "classify_batch", "calc_proj_zoom", "synth_volumes",
    "DataGenerator", "augment_planes", "rotation_params", "GridSearchSVC", "find_best_svm_estimator", "fit_svc",
    "GridSearchSGD", "find_best_sgd_svm_estimator", "fit_sgd", "partial_fit_sgd",
    "partial_fit_sgd_steps", "balance_classes", "balance_indices", "sgd_fit", "svc_fit", "calibrate_prefit", "evaluate_model",
    "ProjMaskSearchSVC", "find_best_proj_mask_svm_estimator", "svc_fit_masks",
    "define_classifier", "train_classifier", "define_discriminator", "fold_batchnorm", "folded_packs",
    "define_generator", "fold_generator", "generator_packs", "generate_dataset",
]


def __getattr__(name):
    # the CNN of dnn.py -- model, fit and the reference's train() -- imported on first use: dnn.py pulls in torch.nn
    if name in ("define_classifier", "train_classifier"):
        from . import dnn
        return dnn.define_classifier if name == "define_classifier" else dnn.train
    # the SGAN classifier (sgan.py): the model whose forward_fused / predict_volumes run csrc/sgan_infer.hip, and its folded weights
    if name in ("define_discriminator", "fold_batchnorm", "folded_packs"):
        from . import sgan
        return getattr(sgan, name)
    # the SGAN generator: the model whose forward_fused / predict(fused=True) run csrc/gen_infer.hip, its folded weights, its data product
    if name in ("define_generator", "fold_generator", "generator_packs", "generate_dataset"):
        from . import sgan
        return getattr(sgan, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
