"""Semi-supervised GAN discriminator / classifier of the reference's ``sgan.py`` (train step) on PyTorch-ROCm.

Architecture (sgan.py:132-217; images/sgan_d_model.png, sgan_c_model.png): per projection branch
3 x [Conv2D(128 / 64 / 32, 3x3, stride 2, 'same') + BatchNorm + LeakyReLU(0.2)] (128 -> 16); concatenate;
Flatten (NHWC, 16*16*96 = 24 576); 2 x [Dense 64 + BatchNorm + LeakyReLU(0.2) + Dropout 0.5]; Dense n_classes.
Two heads on the shared trunk: supervised ``c`` = softmax + sparse categorical cross-entropy; unsupervised
``d`` = custom_activation sum(exp)/(sum(exp)+1) (sgan.py:125-129) + binary cross-entropy.  Each head has its own
Adam(lr 2e-4, beta1 0.5) (sgan.py:206-207,214-215).  Keras semantics kept: TF 'same' padding, NHWC flatten,
RandomNormal(0, 0.02) kernels, zero biases, BatchNorm(momentum 0.99, eps 1e-3) = torch momentum 0.01,
Adam eps 1e-7.  BASELINE config 5: fp16 autocast + loss scaling, data parallel over the GPUs of a node with
DistributedDataParallel (backend "nccl" = RCCL all-reduce of ~1.86 M gradient elements per step);
BatchNorm statistics stay per replica (what Keras does per replica).

The generator side of the loop (sgan.py:57-122, 220-235, 439-543) is here too: :class:`Generator` (three branches of Dense ->
4 x [Conv2DTranspose 4x4 stride 2 + BatchNorm + ReLU] -> Conv2D(1, 7x7, tanh) on one latent input), :class:`GanTrainer`
(``gan_model.train_on_batch``: the generator and -- the reference's quirk -- the discriminator's BatchNorm gammas and betas are
trained, every other discriminator weight is frozen for that step only), ``generate_fake_samples``, the
``generated_data_*.pickle`` product (``generated_samples`` / ``save_generated``) and the four-update loop :func:`train`.  On
the GPU under half-precision autocast the transposed convolutions run through the library -- or, with ``convolutions="hip"``
(``Generator.conv_impl``), on csrc/convt_train.hip with both of their gradients (nn_common.convt4s2) --, BatchNorm + ReLU is the fused op of the
discriminator (slope 0) and the 7x7 one-channel output layer is csrc/gen.hip (nn_common.conv7_tanh).  In inference mode
(``g_model.predict``: the fake samples of every step, the data product) the whole generator can run on csrc/gen_infer.hip --
``Generator.forward_fused``, ``predict(fused=True)``, :func:`generate_dataset`: the BatchNorm layers folded into the transposed
convolutions (:func:`fold_generator`), each of which is four phase GEMMs on the matrix cores; every ``fused`` keyword defaults to False.
"""
import logging
import os
import pickle

import numpy as np

from . import dnn_guard
from . import prep
from .nn_common import make_same_conv, to_nchw, flatten_nhwc, tf_same_pad

RESCALE = (128, 128)        # sgan.py:39
rng = np.random.default_rng(prep.RANDOM_SEED)       # sgan.py:36: the noise draws and the shuffles of preprocess_data / balance_classes
# original (cols, rows) of the radar projections (sgan.py:43-45)
XZ_SIZE = (176, 22)
YZ_SIZE = (176, 31)
XY_SIZE = (31, 22)

logger = logging.getLogger(__name__)

# The margin guard of the classifier (Discriminator.predict_volumes(label_guard=...), forward_guarded; the policy: dnn_guard.py).
# Rows whose top-2 probability gap is below LABEL_GUARD are scored again from exact inputs.  The fused bf16 chain moves a probability
# by up to 8.16e-3 at 128 x 128 planes (the largest "|dp|" tests/test_sgan_infer_gpu.py prints there against the plain float32 layers,
# re-read from one run on an MI355X: 1.0e-4, 6.39e-3 and, on the batch of 70, 8.16e-3), i.e. a gap by twice that:
# 6 x the error, the CNN's factor, = 4.9e-2.  The guard widens
# itself from what it sees, so this only sets where round one starts.
LABEL_GUARD = 5e-2
# Second level: the float32-class trunk (csrc/sgan_x3.hip, bf16 operand pairs) + the float32 LeakyReLU tail; rows whose gap there is
# below this go on to "x6" (three parts per operand), and rows whose x6 gap is below LABEL_GUARD_X6 to float64.  Each level covers at
# least four times the error measured for the stage in front of it (tests/test_sgan_guard_gpu.py asserts that over its case set).
# Measured on an MI355X, one run: |x3 - float64| <= 1.66e-5 and |x6 - float64| <= 1.93e-6 over the case set; on the near-tie rows
# the guard itself re-scored in those tests (2-class models, a last layer of gain 6) |x3 - x6| reached 2.4e-5 and |x6 - float64|
# 3.7e-6 -- more than the CNN's 5e-5 / 1e-5 allow for, so both levels are wider here.  DESIGN.md 3.6c.
LABEL_GUARD_X3 = 2e-4
LABEL_GUARD_X6 = 2e-5
GUARD_STAGES = (dnn_guard.Stage("x3", LABEL_GUARD_X3, True, "rescored", "observed_error"),
                dnn_guard.Stage("x6", LABEL_GUARD_X6, False, "rescored_x6", "observed_error_x3"))

# the fused HIP layers of both models (on by default wherever they apply); `plain_layers()` runs the plain PyTorch layers instead
# -- the library's kernels under the same autocast -- for A/B timings and for the tests that measure one path against the other
_FUSED_LAYERS = True


class plain_layers:
    """``with sgan.plain_layers(): ...``: the discriminator and the generator run their plain PyTorch layers inside the block."""

    def __enter__(self):
        global _FUSED_LAYERS
        self.prev, _FUSED_LAYERS = _FUSED_LAYERS, False
        return self

    def __exit__(self, *exc):
        global _FUSED_LAYERS
        _FUSED_LAYERS = self.prev
        return False


def _nn():
    import torch.nn as nn
    return nn


class Discriminator(dnn_guard.ExactRescore, _nn().Module):
    def __init__(self, shapes=((128, 128, 1),) * 3, n_classes=3):
        nn = _nn()
        super().__init__()
        self.shapes = [tuple(s) for s in shapes]
        self.n_classes = n_classes
        self.branches = nn.ModuleList()
        feat = 0
        for (h, w, c) in self.shapes:
            layers, ch = [], c
            for out in (128, 64, 32):
                layers += [make_same_conv(ch, out, 3, 2), nn.BatchNorm2d(out, eps=1e-3, momentum=0.01), nn.LeakyReLU(0.2)]
                ch = out
                h, w = -(-h // 2), -(-w // 2)
            self.branches.append(nn.Sequential(*layers))
            feat += h * w * 32
        self.flat_features = feat
        self.fc1 = nn.Linear(feat, 64); self.bn1 = nn.BatchNorm1d(64, eps=1e-3, momentum=0.01)
        self.fc2 = nn.Linear(64, 64); self.bn2 = nn.BatchNorm1d(64, eps=1e-3, momentum=0.01)
        self.fc3 = nn.Linear(64, n_classes)
        self.act = nn.LeakyReLU(0.2)
        self.drop = nn.Dropout(0.5)
        # backward of the fused conv + batch-norm layers: zeros for the (cancelled) convolution bias, or no gradient at all
        # (nn_common.fused_step_scope; DiscriminatorTrainer turns the zeros off unless torch's DDP wraps the model)
        self.zero_bias_grads = True
        # the stride-2 convolutions of layers 2 and 3 in the fused training path: "library" (F.conv2d, i.e. MIOpen) or "hip"
        # (nn_common.conv3s2: csrc/conv_train.hip, forward and both gradients; reproducible bit for bit)
        self.conv_impl = "library"
        self._packs = {}                            # name -> (key of the tensors it was made from, value): _cached
        self._margin = dnn_guard.MarginGuard(stages=GUARD_STAGES)
        for mod in self.modules():
            if isinstance(mod, (nn.Conv2d, nn.Linear)):
                nn.init.normal_(mod.weight, 0.0, 0.02)      # RandomNormal(stddev=0.02), sgan.py:176
                nn.init.zeros_(mod.bias)

    @staticmethod
    def _branch(x, br, half=None, conv_impl="library"):
        """[Conv2D 'same' s2 + BatchNorm + LeakyReLU] x 3 (sgan.py:137-158).  On the GPU under half-precision autocast and
        in training mode: batch norm + LeakyReLU + the bottom/right zero pad of the next convolution are one fused HIP op
        (nn_common.bn_lrelu_pad), the convolutions run without their bias (batch norm cancels it; its gradient is exactly
        zero and is handed back as such), and the 1-channel first layer is one autograd node whose backward sums the weight
        gradient without materialising the gradient of the convolution output (nn_common.conv1_bn_lrelu_pad).
        ``conv_impl="hip"``: the other convolutions of that path are nn_common.conv3s2 (csrc/conv_train.hip) instead of F.conv2d.
        Otherwise the plain PyTorch layers run."""
        import torch
        import torch.nn.functional as F
        from .nn_common import bn_lrelu_pad, conv1_bn_lrelu_pad, conv3s2, tf_same_pad
        layers = list(br)
        nlayer = len(layers) // 3
        even = all(s % (2 ** nlayer) == 0 for s in x.shape[-2:])
        adt = torch.get_autocast_dtype("cuda") if (x.is_cuda and torch.is_autocast_enabled("cuda")) else None
        if not (_FUSED_LAYERS and x.is_cuda and br.training and even and adt in (torch.float16, torch.bfloat16)):
            return br(x)
        ph, pw = tf_same_pad(x.shape[-2], 3, 2), tf_same_pad(x.shape[-1], 3, 2)
        # the 1-channel input of the first convolution; tagged channels_last explicitly (for C = 1 the strides alone do
        # not say), otherwise MIOpen answers in NCHW and 268 MB layout copies appear on both sides of layer 1
        x = F.pad(x, (pw[0], pw[1], ph[0], ph[1])).contiguous(memory_format=torch.channels_last)
        for li in range(nlayer):
            conv, bn, act = layers[3 * li].conv, layers[3 * li + 1], layers[3 * li + 2]      # the inner Conv2d: input is padded
            pad = 1 if li + 1 < nlayer else 0
            c = conv.out_channels
            if (li == 0 and conv.in_channels == 1 and not x.requires_grad and x.shape[-1] % 2 == 1 and x.shape[-2] % 2 == 1
                    and c % 8 == 0 and 256 % (c // 8) == 0 and bn.track_running_stats and bn.affine and bn.momentum is not None):
                x = conv1_bn_lrelu_pad(x, conv, bn, act.negative_slope, pad, adt)
                continue
            w = half.get(conv.weight, conv.weight) if half else conv.weight
            z = conv3s2(x, w.to(x.dtype)) if conv_impl == "hip" else F.conv2d(x, w, None, stride=2)
            x = bn_lrelu_pad(z, bn, act.negative_slope, pad=pad, conv_bias=conv.bias)
        return x

    def forward(self, xz, yz, xy):
        """Pre-activation class scores (N, n_classes) -- the shared ``cls`` tensor of sgan.py:199."""
        import torch
        import torch.nn.functional as F
        from .nn_common import cast_all, fused_step_scope
        adt = torch.get_autocast_dtype("cuda") if (xz.is_cuda and torch.is_autocast_enabled("cuda")) else None
        if not (_FUSED_LAYERS and self.training and adt in (torch.float16, torch.bfloat16)):
            outs = [self._branch(x, br, None, self.conv_impl) for x, br in zip((xz, yz, xy), self.branches)]
            fv = flatten_nhwc(torch.cat(outs, dim=1))
            h = self.drop(self.act(self.bn1(self.fc1(fv))))
            h = self.drop(self.act(self.bn2(self.fc2(h))))
            return self.fc3(h)
        # training under half-precision autocast on the GPU: the weights the matrix cores read are cast in one launch (and
        # their gradients cast back in one), the batch-norm bookkeeping of the fused layers is applied in two (nn_common)
        ws = [layers[i].conv.weight for layers in (list(br) for br in self.branches) for i in range(3, len(layers), 3)]
        ws += [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias]
        half = dict(zip(ws, cast_all(adt, *ws)))
        with fused_step_scope(bias_grads=self.zero_bias_grads):
            outs = [self._branch(x, br, half, self.conv_impl) for x, br in zip((xz, yz, xy), self.branches)]
        fv = flatten_nhwc(torch.cat(outs, dim=1))
        h = self.drop(self.act(self.bn1(F.linear(fv, half[self.fc1.weight], half[self.fc1.bias]))))
        h = self.drop(self.act(self.bn2(F.linear(h, half[self.fc2.weight], half[self.fc2.bias]))))
        return F.linear(h, half[self.fc3.weight], half[self.fc3.bias])


    # ---- inference on the fused HIP chain (csrc/sgan_infer.hip + the LeakyReLU tail of csrc/dense.hip) ---------------
    def _cached(self, name, tensors, make):
        """``make()``, kept under ``name`` until one of ``tensors`` is written: the key holds the version counter and the storage
        of every parameter AND every BatchNorm buffer, so an optimizer step, a training-mode forward (``num_batches_tracked``
        advances), ``set_keras_weights``, ``load_state_dict`` or ``.to()`` in between makes the next call rebuild the packs."""
        key = tuple((t._version, t.data_ptr()) for t in tensors)
        hit = self._packs.get(name)
        if hit is None or hit[0] != key:
            hit = self._packs[name] = (key, make())
        return hit[1]

    def folded_packs(self):
        """:func:`folded_packs` of this model, cached (:meth:`_cached`)."""
        return self._cached("folded", list(self.parameters()) + list(self.buffers()), lambda: folded_packs(self))

    def fused_supported(self, H, W):
        """True when the fused inference chain takes (H, W) planes on this model: three one-channel branches of that size,
        H and W multiples of 8, W <= 128 (``rml_sgan_trunk_supported``), the reference's 64 / 64 / n dense layers, n <= 16."""
        from . import _lib
        H, W = int(H), int(W)
        return (len(self.branches) == 3 and all(tuple(sh) == (H, W, 1) for sh in self.shapes) and self.n_classes <= 16
                and bool(_lib.load().rml_sgan_trunk_supported(H, W)))

    def features_fused(self, xz, yz, xy):
        """The flattened trunk output ``flatten_nhwc(cat(branches))`` in inference mode, (N, (H/8)(W/8)*96) bfloat16, from the fused
        HIP trunk (csrc/sgan_infer.hip: BatchNorm folded into the weights, the layer-1 activation recomputed in registers, no
        atomics -- a row depends on its own planes only).  Inputs (N, H, W) or (N, 1, H, W) CUDA tensors, float32 or bfloat16
        (same results).  Raises ValueError for planes the trunk does not take (there is no fall-back)."""
        import torch
        from . import _lib
        H, W = int(xz.shape[-2]), int(xz.shape[-1])
        if not self.fused_supported(H, W):
            raise ValueError("the fused SGAN trunk takes planes of the model's own size (%s) whose height and width are multiples of 8, "
                             "width <= 128: got %dx%d planes" % ("x".join(str(v) for v in self.shapes[0][:2]), H, W))
        if not xz.is_cuda:
            raise RuntimeError("features_fused runs on the GPU (there is no CPU path)")
        lib = _lib.load()
        bf = all(x.dtype == torch.bfloat16 for x in (xz, yz, xy))
        xs = [x.reshape(x.shape[0], x.shape[-2], x.shape[-1]) for x in (xz, yz, xy)]
        xs = [(x if bf else x.float()).contiguous() for x in xs]
        if any(tuple(x.shape) != tuple(xs[0].shape) for x in xs):
            raise ValueError("features_fused: three plane sets of one shape expected")
        n, dev = int(xs[0].shape[0]), xs[0].device
        pk = self.folded_packs()
        feat = torch.empty((n, (H // 8) * (W // 8) * 96), dtype=torch.bfloat16, device=dev)
        if n == 0:
            return feat
        nbytes = int(lib.rml_sgan_trunk_workspace_bytes(n, H, W))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rml_sgan_trunk(_lib.context(dev), _lib.ptr(xs[0]), _lib.ptr(xs[1]), _lib.ptr(xs[2]), 1 if bf else 0, n, H, W,
                                          _lib.ptr(pk["w1"]), _lib.ptr(pk["b1"]), _lib.ptr(pk["w2t"]), _lib.ptr(pk["b2"]),
                                          _lib.ptr(pk["w3t"]), _lib.ptr(pk["b3"]), float(pk["slope"]), _lib.ptr(feat), _lib.ptr(ws), nbytes,
                                          _lib.stream_ptr(dev)), "rml_sgan_trunk")
        return feat

    def dense_tail_fused(self, fv):
        """Dense 64 + BatchNorm + LeakyReLU, twice, Dense n, softmax (inference: no dropout) on bf16 feature rows: csrc/dense.hip's
        split-K first layer and finishing kernel with LeakyReLU (``rml_dense_tail_lrelu``); the BatchNorm1d layers are folded into
        the dense kernels.  (N, n_classes) float32 probabilities."""
        import torch
        from . import _lib
        lib = _lib.load()
        pk = self.folded_packs()
        n, K, dev = int(fv.shape[0]), int(fv.shape[1]), fv.device
        if not (fv.is_cuda and fv.dtype == torch.bfloat16 and fv.ndim == 2 and fv.is_contiguous() and K % 64 == 0
                and tuple(pk["fc1_w"].shape) == (64, K) and tuple(pk["fc2_wt"].shape) == (64, 64) and self.n_classes <= 16):
            raise ValueError("dense_tail_fused: contiguous CUDA bfloat16 (N, %d) feature rows expected" % int(pk["fc1_w"].shape[1]))
        out = torch.empty((n, self.n_classes), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        ctx = _lib.context(dev)
        nbytes = int(lib.rml_dnn_dense_workspace_bytes(ctx, n, K))
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rml_dense_tail_lrelu(ctx, _lib.ptr(fv), K, n, K, _lib.ptr(pk["fc1_w"]), _lib.ptr(pk["fc1_b"]), _lib.ptr(pk["fc2_wt"]),
                                                _lib.ptr(pk["fc2_b"]), _lib.ptr(pk["fc3_w"]), _lib.ptr(pk["fc3_b"]), self.n_classes,
                                                float(pk["slope"]), _lib.ptr(ws), nbytes, _lib.ptr(out), _lib.stream_ptr(dev)),
                       "rml_dense_tail_lrelu")
        return out

    def forward_fused(self, xz, yz, xy):
        """``softmax(c_model)`` in inference mode on the fused HIP chain: (N, n_classes) float32 class probabilities on the device
        from float32 or bfloat16 planes (same results).  Raises for planes the trunk does not take."""
        import torch
        with torch.no_grad():
            return self.dense_tail_fused(self.features_fused(xz, yz, xy))

    # ---- exact-input arithmetic: what the margin guard re-scores with (csrc/sgan_x3.hip + the float32 LeakyReLU tail of csrc/dense.hip) --
    def x3_supported(self, H, W):
        """True when csrc/sgan_x3.hip takes (H, W) planes on this model: three one-channel branches of that size, H and W multiples of
        8 (``rml_sgan_trunk_x3_supported``), the reference's 64 / 64 / n dense layers, n <= 16."""
        from . import _lib
        H, W = int(H), int(W)
        return (len(self.branches) == 3 and all(tuple(sh) == (H, W, 1) for sh in self.shapes) and self.n_classes <= 16
                and bool(_lib.load().rml_sgan_trunk_x3_supported(H, W)))

    def features_x3(self, xz, yz, xy, parts=2):
        """The flattened trunk output in float32 from the float32-class trunk (csrc/sgan_x3.hip): (N,H,W) or (N,1,H,W) CUDA float32
        planes -> (N, (H/8)(W/8)*96) rows in Keras' Flatten order, the BatchNorm layers folded in (float64 fold, one cast to float32).
        ``parts`` = 2: ~2^-16 relative per product (bf16 pairs, three matrix-core products each, "x3"); 3: ~2^-24 (bf16 triples, six
        products, "x6").  A row depends on its own planes only.  Raises ValueError for planes the kernel does not take."""
        import torch
        from . import _lib
        H, W = int(xz.shape[-2]), int(xz.shape[-1])
        if not self.x3_supported(H, W):
            raise ValueError("the float32-class SGAN trunk takes planes of the model's own size (%s) whose height and width are multiples "
                             "of 8: got %dx%d planes" % ("x".join(str(v) for v in self.shapes[0][:2]), H, W))
        if not xz.is_cuda:
            raise RuntimeError("features_x3 runs on the GPU (there is no CPU path)")
        lib = _lib.load()
        xs = [x.reshape(x.shape[0], x.shape[-2], x.shape[-1]).float().contiguous() for x in (xz, yz, xy)]
        if any(tuple(x.shape) != tuple(xs[0].shape) for x in xs):
            raise ValueError("features_x3: three plane sets of one shape expected")
        n, dev = int(xs[0].shape[0]), xs[0].device
        pk = self.folded_packs()
        feat = torch.empty((n, (H // 8) * (W // 8) * 96), dtype=torch.float32, device=dev)
        if n == 0:
            return feat
        nbytes = int(lib.rml_sgan_trunk_x3_workspace_bytes(n, H, W))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rml_sgan_trunk_x3(_lib.context(dev), _lib.ptr(xs[0]), _lib.ptr(xs[1]), _lib.ptr(xs[2]), n, H, W,
                                             _lib.ptr(pk["w1"]), _lib.ptr(pk["b1"]), _lib.ptr(pk["w2f"]), _lib.ptr(pk["b2"]),
                                             _lib.ptr(pk["w3f"]), _lib.ptr(pk["b3"]), float(pk["slope"]), int(parts), _lib.ptr(feat),
                                             _lib.ptr(ws), nbytes, _lib.stream_ptr(dev)), "rml_sgan_trunk_x3")
        return feat

    def _tail_float32(self, fv):
        """Dense 64 + BatchNorm + LeakyReLU, twice, Dense n, softmax in float32 on float32 CUDA feature rows (inference: no dropout;
        the BatchNorm1d layers folded in): csrc/dense.hip ``rml_dense_tail_lrelu_f32`` -- fixed K splits added in order, so a row
        scored alone, inside any candidate set or twice has the same bits."""
        import torch
        from . import _lib
        lib = _lib.load()
        pk = self.folded_packs()
        n, K, dev = int(fv.shape[0]), int(fv.shape[1]), fv.device
        if not (fv.is_cuda and fv.dtype == torch.float32 and fv.ndim == 2 and fv.is_contiguous() and K % 4 == 0
                and tuple(pk["fc1_wf"].shape) == (64, K) and tuple(pk["fc2_wt"].shape) == (64, 64) and self.n_classes <= 16):
            raise ValueError("_tail_float32: contiguous CUDA float32 (N, %d) feature rows expected" % int(pk["fc1_wf"].shape[1]))
        out = torch.empty((n, self.n_classes), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        nbytes = int(lib.rml_dnn_dense_tail_f32_workspace_bytes(n, K))
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rml_dense_tail_lrelu_f32(_lib.context(dev), _lib.ptr(fv), K, n, K, _lib.ptr(pk["fc1_wf"]), _lib.ptr(pk["fc1_b"]),
                                                    _lib.ptr(pk["fc2_wt"]), _lib.ptr(pk["fc2_b"]), _lib.ptr(pk["fc3_w"]), _lib.ptr(pk["fc3_b"]),
                                                    self.n_classes, float(pk["slope"]), _lib.ptr(ws), nbytes, _lib.ptr(out),
                                                    _lib.stream_ptr(dev)), "rml_dense_tail_lrelu_f32")
        return out

    def _eval_layers(self, xs):
        """The plain PyTorch layers in inference mode whatever ``self.training`` says (BatchNorm on its moving statistics, no dropout):
        (N,1,H,W) planes -> probabilities in the planes' dtype."""
        import torch
        import torch.nn.functional as F

        def bn(x, m):
            return F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
        outs = []
        for x, br in zip(xs, self.branches):
            layers = list(br)
            for i in range(0, len(layers), 3):
                x = F.leaky_relu(bn(layers[i](x), layers[i + 1]), layers[i + 2].negative_slope)
            outs.append(x)
        slope = self.act.negative_slope
        h = F.leaky_relu(bn(self.fc1(flatten_nhwc(torch.cat(outs, dim=1))), self.bn1), slope)
        h = F.leaky_relu(bn(self.fc2(h), self.bn2), slope)
        return torch.softmax(self.fc3(h), dim=-1)

    def _folded64(self):
        """:func:`fold_batchnorm` of this model (float64), cached like the packs"""
        return self._cached("folded64", list(self.parameters()) + list(self.buffers()), lambda: fold_batchnorm(self))

    def features_float64(self, xz, yz, xy):
        """The flattened trunk output of the :func:`fold_batchnorm` model in float64 on the inputs' device, (N, (H/8)(W/8)*96): each
        convolution as im2col -- nine strided slices -- and a matrix product, as ``dnn.Classifier.forward_exact`` does it (MIOpen has
        no float64 convolution)."""
        import torch
        import torch.nn.functional as F
        f = self._folded64()
        slope, dt = f["slope"], torch.float64
        with torch.no_grad():
            outs = []
            for x, convs in zip((xz, yz, xy), f["conv"]):
                x = x.reshape(x.shape[0], 1, x.shape[-2], x.shape[-1]).to(dt)
                for w, b in convs:
                    kh, kw = int(w.shape[2]), int(w.shape[3])
                    ph, pw = tf_same_pad(x.shape[-2], kh, 2), tf_same_pad(x.shape[-1], kw, 2)
                    oh, ow = -(-x.shape[-2] // 2), -(-x.shape[-1] // 2)
                    xp = F.pad(x, (pw[0], pw[1], ph[0], ph[1]))
                    # (N, Cin, kh*kw, oh, ow) -> (N, Cin*kh*kw, oh*ow): the (cin, ky, kx) order of w.reshape(Cout, -1)
                    cols = torch.stack([xp[:, :, ky:ky + 2 * oh - 1:2, kx:kx + 2 * ow - 1:2] for ky in range(kh) for kx in range(kw)], dim=2)
                    cols = cols.reshape(x.shape[0], -1, oh * ow)
                    x = F.leaky_relu(torch.matmul(w.reshape(w.shape[0], -1), cols) + b[None, :, None], slope).reshape(x.shape[0], w.shape[0], oh, ow)
                outs.append(x)
            return flatten_nhwc(torch.cat(outs, dim=1))

    def forward_exact(self, xz, yz, xy, precision="float64"):
        """``softmax(c_model)`` of sgan.py:132-199 in inference mode (whatever ``self.training`` says) on the inputs' device with no
        single-bf16 operand anywhere: (N,H,W) or (N,1,H,W) planes -> (N, n_classes) probabilities.
        "x3" / "x6": the float32-class HIP trunk (:meth:`features_x3`, two / three bf16 parts per operand) + the float32 LeakyReLU
        tail (:meth:`_tail_float32`) -- the margin guard's first two stages; planes the kernel does not take (and CPU tensors) fall
        to "float32".  "float32": the plain PyTorch layers with autocast off, the reference's own arithmetic.  "float64": the
        :func:`fold_batchnorm` model (float64): :meth:`features_float64` and the dense layers."""
        import torch
        import torch.nn.functional as F
        if precision not in ("x3", "x6", "float32", "float64"):
            raise ValueError("precision must be 'x3', 'x6', 'float32' or 'float64'")
        with torch.no_grad():
            if precision != "float64":
                with torch.autocast("cuda", enabled=False):
                    xs = [x.reshape(x.shape[0], 1, x.shape[-2], x.shape[-1]).float() for x in (xz, yz, xy)]
                    if precision in ("x3", "x6") and xs[0].is_cuda and self.x3_supported(xs[0].shape[-2], xs[0].shape[-1]):
                        return self._tail_float32(self.features_x3(*xs, parts=3 if precision == "x6" else 2))
                    return self._eval_layers(xs)
            f = self._folded64()
            slope = f["slope"]
            h = self.features_float64(xz, yz, xy)
            (w1, b1), (w2, b2), (w3, b3) = f["fc"]
            # the first dense layer as a batch of K-slices and a sum (rocBLAS' float64 GEMM with a few rows and a long K runs on a
            # handful of workgroups: dnn.Classifier.forward_exact)
            K = int(h.shape[1])
            kc = 256 if K % 256 == 0 else K
            part = torch.bmm(h.reshape(h.shape[0], K // kc, kc).transpose(0, 1), w1.reshape(w1.shape[0], K // kc, kc).permute(1, 2, 0))
            h = F.leaky_relu(part.sum(dim=0) + b1, slope)
            h = F.leaky_relu(F.linear(h, w2, b2), slope)
            return torch.softmax(F.linear(h, w3, b3), dim=-1)

    def rescore_exact(self, volumes, rescale=RESCALE, mode="max", precision="float64", rows=None, ijk=None):
        """(n,X,Y,Z) volumes -> (n, n_classes) probabilities without a rounding the reference does not have: exact projection
        (``common.process_volumes(scale=False)``), (p - 127.5) / 127.5 and Pillow's bicubic resize to float32 planes as Pillow stores
        them (csrc/resize.hip, bit-identical), then :meth:`forward_exact` in ``precision``.  ``rows``: an index tensor -- score
        ``volumes[rows]`` in that order; ``mode="slice"``: ``ijk`` (n,3) or (n,T,3), the result has n*T rows, frame-major, ``rows``
        indexes those and row r is scored from frame r // T at ijk[r].  Bounded passes, host or device volumes: the passes are
        dnn_guard.ExactRescore's, shared with the CNN."""
        return self._rescore(volumes, rescale, mode, precision, rows, ijk)

    @property
    def last_guard(self):
        """What the last guarded call did (the keys: dnn_guard.py); None before the first one."""
        return self._margin.last

    def _guard(self, proba, eps, rescore):
        """dnn_guard.MarginGuard with this model's stage thresholds (LABEL_GUARD_X3, LABEL_GUARD_X6) on dnn_guard.CudaOps: the rows of
        ``proba`` whose top-2 gap is below ``eps`` are replaced by what ``rescore(rows, precision)`` gives."""
        return self._margin.run(proba, eps, rescore, dnn_guard.CudaOps(), list(self.parameters()) + list(self.buffers()))

    def forward_guarded(self, xz, yz, xy, label_guard=LABEL_GUARD):
        """:meth:`forward_fused` with the margin guard on float32 planes: rows whose two largest probabilities are closer than
        ``label_guard`` are scored again on the planes themselves through :meth:`forward_exact` ("x3", then "x6", then "float64" for
        the rows that stay near a tie) and replaced, so that ``argmax`` is the float64 label (the bound is empirical: dnn_guard.py).
        ``label_guard`` None or 0: exactly :meth:`forward_fused`.  ``self.last_guard``: what the guard did."""
        import torch
        p = self.forward_fused(xz, yz, xy)
        if not label_guard:
            self._margin.run(p, None, None, None, ())
            return p
        xs = [x.reshape(x.shape[0], x.shape[-2], x.shape[-1]) for x in (xz, yz, xy)]
        with torch.no_grad(), torch.cuda.device(p.device):
            return self._guard(p, label_guard, lambda idx, prec: self.forward_exact(*[x[idx] for x in xs], precision=prec))

    def predict_volumes(self, volumes, rescale=RESCALE, mode="max", ijk=None, batch_size=8192, exact_resize=False, return_numpy=True,
                        num_targets=1, return_ijk=False, label_guard=None):
        """Radar volumes -> class probabilities on the GPU: (N, X, Y, Z) volumes (float32 or uint8; numpy or torch, host or device)
        -> projections -> ``(p - 127.5) / 127.5`` and the bicubic resize of sgan.py:636-681 to ``rescale`` (Pillow's (width, height))
        -> fused trunk -> LeakyReLU tail.  Grids the fused preprocessing kernel takes (``nn_common.preprocess_supported``: at 128x128 the
        Walabot grid does, 64x64x128 does not) go from uint8 code rows to bf16 planes in one launch (Pillow's windows in float32: the planes are within one bf16 ulp
        of the exact ones); other grids, mode "max_nan" and ``exact_resize=True`` take float32 rows and the Pillow-bit-identical
        resize.  ``mode="slice"``: the planes through a target's voxel (predict.py:98-107) at ``ijk`` (N,3) or -- every target of every
        frame, predict.py:93-119 -- (N,T,3); ``ijk=None``: the ``num_targets`` strongest derived targets of every frame.  The result has
        N*T rows, frame-major (row b*T+t), (N,T,3) and derived targets in one preprocessing launch straight from the volumes
        (csrc/preprocess_slice.hip); ``return_ijk=True`` returns ``(proba, ijk)`` with the (N,T,3) int32 indices used (a CUDA tensor;
        NumPy with ``return_numpy``).  ``batch_size``: frames per pass; a row's result does not depend on it.
        ``label_guard`` (None or 0: off, the default -- the chain above and its bits): the margin guard (dnn_guard.py), once per call
        behind the last pass, for every mode.  The bf16 chain moves a probability by a few 1e-3 (up to 8.2e-3 measured), so rows
        whose two largest probabilities are closer than ``label_guard`` (``sgan.LABEL_GUARD``) are scored again from their volumes
        from exact inputs (:meth:`rescore_exact`: "x3", then "x6", then "float64" for the rows that stay near a tie; slice rows from
        frame r // T at the indices used) and replaced; the gap widens itself to four times the error seen.  ``argmax`` is then the
        float64 label on every row inside the covered gap -- an empirical bound, as the CNN's.  Guarded results are not
        batching-invariant bit for bit; unguarded ones are.  ``self.last_guard``: what the guard did."""
        import torch
        from . import common, nn_common
        if not isinstance(volumes, torch.Tensor):
            volumes = torch.as_tensor(np.asarray(volumes))
        n = int(volumes.shape[0])
        dev = volumes.device if volumes.is_cuda else next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("predict_volumes runs on the GPU: move the model to a CUDA device (there is no CPU path)")
        oh, ow = int(rescale[1]), int(rescale[0])
        if not self.fused_supported(oh, ow):
            raise ValueError("predict_volumes: the fused SGAN trunk does not take %dx%d planes on this model" % (oh, ow))
        sliced = mode == "slice"
        T = 1
        if sliced:
            ijk, T = nn_common.slice_targets_arg(ijk, n, num_targets)
        out = torch.empty((n * T, self.n_classes), dtype=torch.float32, device=dev)
        dims = tuple(int(v) for v in volumes.shape[1:])
        fused = not exact_resize and mode != "max_nan" and nn_common.preprocess_supported(dims, rescale)
        bs = max(1, int(batch_size))
        used = []
        with torch.no_grad(), torch.cuda.device(dev):
            for s0 in range(0, n, bs):
                s1 = min(n, s0 + bs)
                v = volumes[s0:s1] if volumes.is_cuda else volumes[s0:s1].to(dev)
                if v.dtype != torch.uint8:
                    v = v.float()
                idx = None if ijk is None else ijk[s0:s1]
                if fused:
                    xs = nn_common.preprocess_volumes(v, rescale, mode=mode, ijk=idx, num_targets=T, return_ijk=sliced)
                    if sliced:
                        xs, got = xs
                else:
                    feat = common.process_volumes(v, mode=mode, ijk=idx, num_targets=T, scale=False, return_ijk=sliced)
                    if sliced:
                        feat, got = feat
                    xs = nn_common.preprocess_features(feat, dims, rescale, out_dtype="bfloat16")
                if sliced:
                    used.append(got)
                out[s0 * T:s1 * T] = self.forward_fused(*xs)
            if label_guard:
                vol = volumes if volumes.dtype in (torch.uint8, torch.float32) else volumes.float()
                at = (torch.cat(used) if len(used) != 1 else used[0]) if sliced else None
                out = self._guard(out, label_guard, lambda idx, prec: self.rescore_exact(vol, rescale, mode, prec, rows=idx, ijk=at))
        res = out.cpu().numpy() if return_numpy else out
        if sliced and return_ijk:
            got = torch.cat(used) if used else torch.zeros((0, T, 3), dtype=torch.int32, device=dev)
            return res, (got.cpu().numpy() if return_numpy else got)
        return res

    # ---- Keras layout in / out -------------------------------------------------------------------------
    def _conv_bn_pairs(self):
        out = []
        for br in self.branches:
            layers = list(br)
            out.append([(layers[i].conv, layers[i + 1]) for i in range(0, len(layers), 3)])
        return out

    def keras_weights(self):
        """The parameters AND BatchNorm statistics in Keras layout, float64 numpy:
        ``(branches, dense)`` with branches[b] = [(kernel (kh,kw,cin,cout), bias, gamma, beta, moving_mean, moving_variance)] x 3
        and dense = [(kernel (in,out), bias, gamma, beta, moving_mean, moving_variance)] x 2 + [(kernel, bias)] --
        what ``layer.get_weights()`` of the reference's c_model / d_model holds layer by layer (sgan.py:132-199;
        Keras BatchNormalization lists gamma, beta, moving_mean, moving_variance)."""
        def a(t):
            return t.detach().double().cpu().numpy()

        def bn4(bn):
            return a(bn.weight), a(bn.bias), a(bn.running_mean), a(bn.running_var)
        branches = [[(a(conv.weight.permute(2, 3, 1, 0)), a(conv.bias)) + bn4(bn) for conv, bn in pairs] for pairs in self._conv_bn_pairs()]
        dense = [(a(self.fc1.weight.t()), a(self.fc1.bias)) + bn4(self.bn1), (a(self.fc2.weight.t()), a(self.fc2.bias)) + bn4(self.bn2),
                 (a(self.fc3.weight.t()), a(self.fc3.bias))]
        return branches, dense

    def set_keras_weights(self, branches, dense):
        """Inverse of :meth:`keras_weights`: what a maintainer pulls out of a trained ``c_model_XXXX.h5`` (sgan.py:496-500)
        goes in here; the moving statistics land in the BatchNorm buffers, so inference (``predict`` / ``evaluate``)
        reproduces the Keras model."""
        import torch
        pairs = self._conv_bn_pairs()
        if len(branches) != len(pairs) or len(dense) != 3:
            raise ValueError("expected %d branches of 3 (conv + batch-norm) tuples and 3 dense tuples" % len(pairs))

        def put(dst, arr, what):
            t = torch.as_tensor(np.asarray(arr), dtype=dst.dtype)
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError("%s: Keras array gives %s, the layer holds %s" % (what, tuple(t.shape), tuple(dst.shape)))
            dst.copy_(t.to(dst.device))

        def put_bn(bn, g, b, mean, var, what):
            put(bn.weight, g, what + " gamma"); put(bn.bias, b, what + " beta")
            put(bn.running_mean, mean, what + " moving_mean"); put(bn.running_var, var, what + " moving_variance")

        with torch.no_grad():
            for bi, (prs, given) in enumerate(zip(pairs, branches)):
                if len(given) != len(prs):
                    raise ValueError("branch %d: expected %d (conv + batch-norm) tuples" % (bi, len(prs)))
                for li, ((conv, bn), (k, b, g, be, mu, var)) in enumerate(zip(prs, given)):
                    what = "branch %d layer %d" % (bi, li)
                    put(conv.weight, np.asarray(k).transpose(3, 2, 0, 1), what + " kernel")
                    put(conv.bias, b, what + " bias")
                    put_bn(bn, g, be, mu, var, what)
            for fc, bn, tup, nm in ((self.fc1, self.bn1, dense[0], "dense"), (self.fc2, self.bn2, dense[1], "dense_1")):
                k, b, g, be, mu, var = tup
                put(fc.weight, np.asarray(k).T, nm + " kernel"); put(fc.bias, b, nm + " bias")
                put_bn(bn, g, be, mu, var, nm)
            k, b = dense[2]
            put(self.fc3.weight, np.asarray(k).T, "dense_2 kernel"); put(self.fc3.bias, b, "dense_2 bias")
        return self


def fold_batchnorm(model):
    """The inference-mode model with every BatchNorm folded into the layer in front of it, float64 on the model's device:
    ``s = gamma / sqrt(moving_variance + eps)``, ``w' = w * s`` (per output channel / unit), ``b' = beta + (bias - moving_mean) * s``.
    Returns ``{"conv": [[(w (out, in, 3, 3), b)] x 3 per branch], "fc": [(w (out, in), b)] x 3, "slope": LeakyReLU slope}``; a layer is
    then ``LeakyReLU(conv_same_stride2(x, w) + b)`` / ``LeakyReLU(x @ w.T + b)`` and the last one ``x @ w.T + b``."""
    def fold(w, b, bn):
        sc = bn.weight.detach().double() / (bn.running_var.detach().double() + float(bn.eps)).sqrt()
        wf = w.detach().double() * sc.reshape((-1,) + (1,) * (w.ndim - 1))
        return wf, bn.bias.detach().double() + (b.detach().double() - bn.running_mean.detach().double()) * sc
    conv = [[fold(cv.weight, cv.bias, bn) for cv, bn in pairs] for pairs in model._conv_bn_pairs()]
    fc = [fold(model.fc1.weight, model.fc1.bias, model.bn1), fold(model.fc2.weight, model.fc2.bias, model.bn2),
          (model.fc3.weight.detach().double(), model.fc3.bias.detach().double())]
    return {"conv": conv, "fc": fc, "slope": float(model.act.negative_slope)}


def folded_packs(model):
    """:func:`fold_batchnorm` in the layouts of ``rml_sgan_trunk`` and ``rml_dense_tail_lrelu``, computed in float64 and cast once, on
    the model's device (CPU tensors for a CPU model): ``w1`` (3, 128, 9) and ``b1`` (3, 128) float32; ``w2t`` (3, 64, 1152) and ``w3t``
    (3, 32, 576) bfloat16 with k = (ky * 3 + kx) * Cin + cin, ``b2`` (3, 64) and ``b3`` (3, 32) float32; ``fc1_w`` (64, K) bfloat16 in
    Keras' row order, ``fc1_b``; ``fc2_wt`` (64 in, 64 out), ``fc2_b``, ``fc3_w`` (n, 64), ``fc3_b`` float32; ``slope``.  Three branches of
    one-channel planes expected (the reference's model)."""
    import torch
    f = fold_batchnorm(model)
    if len(f["conv"]) != 3 or any(len(br) != 3 or br[0][0].shape[1] != 1 for br in f["conv"]):
        raise ValueError("folded_packs: three branches of three convolutions on one-channel planes expected")

    def taps(w):            # (out, in, ky, kx) -> (out, ky, kx, in) -> (out, 9 * in)
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    st = lambda li, what, dt: torch.stack([(taps(br[li][0]) if what == "w" else br[li][1]) for br in f["conv"]]).to(dt).contiguous()
    (w1, b1), (w2, b2), (w3, b3) = f["fc"]
    return {"w1": st(0, "w", torch.float32), "b1": st(0, "b", torch.float32),
            "w2t": st(1, "w", torch.bfloat16), "b2": st(1, "b", torch.float32),
            "w3t": st(2, "w", torch.bfloat16), "b3": st(2, "b", torch.float32),
            "w2f": st(1, "w", torch.float32), "w3f": st(2, "w", torch.float32), "fc1_wf": w1.float().contiguous(),
            "fc1_w": w1.to(torch.bfloat16).contiguous(), "fc1_b": b1.float().contiguous(),
            "fc2_wt": w2.float().t().contiguous(), "fc2_b": b2.float().contiguous(),
            "fc3_w": w3.float().contiguous(), "fc3_b": b3.float().contiguous(), "slope": f["slope"]}


def class_weight_to_sample_weight(y, class_weight):
    """``train_on_batch(..., class_weight=w)`` as Keras applies it (sgan.py:529-530 passes the data set's class weights to
    the d update): the target is cast to an integer class, ``int(y)`` truncating toward zero -- the smoothed real labels in
    [0.7, 1.2) of sgan.py:396-398 therefore select class 0 or 1 -- and that class's weight becomes the sample's weight
    (classes missing from the dict weigh 1)."""
    yi = np.trunc(np.asarray(y, dtype=np.float64).reshape(-1)).astype(np.int64)
    w = np.ones(len(yi), dtype=np.float32)
    for cls, val in dict(class_weight).items():
        w[yi == int(cls)] = float(val)
    return w


def custom_activation(logits):
    """sgan.py:125-129: sum(exp)/(sum(exp)+1) = sigmoid(logsumexp(logits))."""
    import torch
    return torch.sigmoid(torch.logsumexp(logits.float(), dim=-1, keepdim=True))


def c_loss(logits, y):
    """sparse_categorical_crossentropy on the softmax head (sgan.py:205)."""
    import torch.nn.functional as F
    return F.cross_entropy(logits.float(), y)


def d_loss(logits, y, sample_weight=None):
    """binary_crossentropy on the custom-activation head (sgan.py:213), evaluated on the logit
    lse = logsumexp(logits): -y log D - (1-y) log(1-D) = softplus(lse) - y*lse.  Labels may be smoothed
    floats outside [0,1] (sgan.py:396-403)."""
    import torch
    import torch.nn.functional as F
    lse = torch.logsumexp(logits.float(), dim=-1)
    loss = F.softplus(lse) - y.float().reshape(-1) * lse
    if sample_weight is not None:
        loss = loss * sample_weight.float().reshape(-1)
    return loss.mean()


class DiscriminatorTrainer:
    """c_model / d_model ``train_on_batch`` (sgan.py:525-532) with the reference's optimizers, fp16 autocast and,
    when torch.distributed is initialised, DistributedDataParallel gradient all-reduce."""

    def __init__(self, model, lr=2e-4, beta1=0.5, amp_dtype="float16", ddp=None, use_graph=False, tune_convolutions=False,
                 convolutions="library"):
        """``convolutions``: "library" (default) leaves the model's layer-2 and layer-3 convolutions to ``F.conv2d``; "hip" runs them and
        their gradients on csrc/conv_train.hip (``model.conv_impl``; nn_common.conv3s2): no convolution library, no workspace zeroing,
        and a step that gives the same bits on every run.  Every update that goes through the model follows it -- c, d, d on fakes,
        the generator update of :class:`GanTrainer`, graph replay and both ddp modes.  Any other value: ValueError.

        ``use_graph``: capture forward + backward of each head in a HIP graph (torch.cuda.graphs) after three eager
        warm-up steps and replay it afterwards; the optimizer, the loss scaler and the gradient all-reduce stay outside
        the graph.  Inputs must keep their shapes.  With the fused layers the step is launch-bound on the host side,
        which is what the graph removes.

        ``ddp``: data parallelism when torch.distributed is initialised with more than one rank (None = on).  The
        replicas are kept in step the MI355X way: every parameter's ``.grad`` is a view into ONE flat float32 bucket
        (1.86 M elements = 7.4 MB) that is all-reduced (RCCL over xGMI; gloo on CPU) once per update, after the
        backward pass and before the loss-scaled optimizer step -- a single collective of a few tens of microseconds
        instead of per-bucket hooks inside the backward, so forward + backward can still be replayed from a HIP graph.
        ``ddp="torch"`` wraps the model in torch's DistributedDataParallel instead (no graph replay then).
        BatchNorm statistics stay per replica (what Keras does per replica).

        ``tune_convolutions``: runs this trainer's steps with ``torch.backends.cudnn.benchmark = True`` (set around each step and
        restored afterwards: the flag is process-wide and changes which MIOpen kernels -- and so which round-off -- every other
        convolution in the process gets): MIOpen then times its solvers for every convolution shape on first use instead of taking
        its heuristic pick -- a few seconds once, 3 % off the step on an MI355X (a CK xdl forward kernel and a smaller-tile
        weight-gradient kernel win)."""
        import torch
        import torch.distributed as dist
        if convolutions not in ("library", "hip"):
            raise ValueError("convolutions must be 'library' or 'hip', got %r" % (convolutions,))
        model.conv_impl = convolutions
        self._tune = bool(tune_convolutions)
        self.model = model
        self.device = next(model.parameters()).device
        self.net = model
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.world = dist.get_world_size() if multi else 1
        mode = ddp
        if mode is None or mode is True:
            mode = "flat" if multi else None
        elif mode is False:
            mode = None
        if mode is not None and not multi:
            mode = None
        self.ddp_mode = mode
        self._flat = None
        model.zero_bias_grads = mode == "torch"         # DDP wants a gradient for every parameter; Adam does not (exactly zero)
        if mode == "torch":
            from torch.nn.parallel import DistributedDataParallel as DDP
            self.net = DDP(model, device_ids=[self.device.index] if self.device.type == "cuda" else None,
                           gradient_as_bucket_view=True)
        elif mode == "flat":
            with torch.no_grad():                       # identical replicas to start from (what DDP's constructor does)
                for t in list(model.parameters()) + list(model.buffers()):
                    dist.broadcast(t.data, src=0)
            params = [p for p in model.parameters() if p.requires_grad]
            self._flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=self.device)
            off = 0
            for p in params:
                if p.dtype != torch.float32:
                    raise TypeError("flat gradient bucket: float32 master parameters expected")
                # the view takes the parameter's own strides (channels_last convolution kernels): the fused Adam and autograd's
                # gradient-layout contract want grad and param laid out alike
                p.grad = torch.as_strided(self._flat, p.size(), p.stride(), storage_offset=off)
                off += p.numel()
        elif mode is not None:
            raise ValueError("ddp must be None, False, 'flat' or 'torch'")
        # Adam(lr=0.0002, beta_1=0.5), Keras epsilon 1e-7 (sgan.py:206,214); one fused update kernel on the GPU
        # (the per-parameter kernels of the default implementation were 8 % of the step)
        fused = self.device.type == "cuda"
        self.opt_c = torch.optim.Adam(model.parameters(), lr=lr, betas=(beta1, 0.999), eps=1e-7, fused=fused)
        self.opt_d = torch.optim.Adam(model.parameters(), lr=lr, betas=(beta1, 0.999), eps=1e-7, fused=fused)
        self.amp_dtype = getattr(torch, amp_dtype) if (amp_dtype and self.device.type == "cuda") else None
        self.scaler = torch.amp.GradScaler("cuda", enabled=self.amp_dtype == torch.float16)
        self.use_graph = bool(use_graph) and self.device.type == "cuda" and mode != "torch"
        self._params = [q for q in model.parameters() if q.requires_grad]
        # on the GPU the update itself and the loss-scale rule run as three launches over all parameters (nn_common.DeviceAdam,
        # csrc/optim.hip); opt_c / opt_d stay the description of the optimizers (and the CPU path).  RML_DEVICE_ADAM=0: torch's.
        self._dev_adam = None
        if self.device.type == "cuda" and mode != "torch" and os.environ.get("RML_DEVICE_ADAM", "1") != "0":
            from .nn_common import DeviceAdam
            self._scale_t = torch.full((1,), 65536.0, dtype=torch.float32, device=self.device) if self.amp_dtype == torch.float16 else None
            shared = torch.zeros((3,), dtype=torch.int32, device=self.device)
            self._dev_adam = {id(o): DeviceAdam(self._params, lr, (beta1, 0.999), 1e-7, scale=self._scale_t, scaler_state=shared, mirror=o)
                              for o in (self.opt_c, self.opt_d)}
        self._graphs = {}           # head -> dict(graph, static inputs / targets, loss, logits, eager_calls)

    def _scaled(self, loss):
        if self._dev_adam is not None:
            return loss if self._scale_t is None else loss * self._scale_t
        return self.scaler.scale(loss)

    def _opt_step(self, opt):
        if self._dev_adam is not None:
            self._dev_adam[id(opt)].step()
            return
        self.scaler.step(opt)
        self.scaler.update()

    def _zero_grad(self, opt):
        if self._flat is not None:
            self._flat.zero_()          # the grads are views of the bucket: keep them, clear them in one kernel
        else:
            opt.zero_grad(set_to_none=not self.use_graph)

    def _allreduce_grads(self):
        """mean of the (loss-scaled) gradients over the replicas: one collective on the flat bucket.  An overflow on any
        rank reaches every rank through the sum, so the loss scaler skips the step everywhere."""
        if self._flat is None:
            return
        import torch.distributed as dist
        dist.all_reduce(self._flat, op=dist.ReduceOp.SUM)
        self._flat.mul_(1.0 / self.world)

    def _graph_step_impl(self, head, opt, make_loss, x, targets):
        """One update of ``head`` ('c' or 'd') through a captured graph.  ``targets``: tuple of tensors the loss needs
        (copied into static buffers); ``make_loss(logits, *static_targets)`` builds the loss."""
        import torch
        st = self._graphs.setdefault(head, {"eager": 0})
        xs = self._inputs(x)
        key = tuple(tuple(t.shape) for t in xs) + tuple(tuple(t.shape) for t in targets)
        if st.get("key") not in (None, key):            # shapes changed: start over
            st.clear(); st["eager"] = 0
        st["key"] = key
        self.net.train()
        if "graph" not in st:
            if st["eager"] < 3:                         # eager warm-up (MIOpen find, allocator, lazy initialisations)
                st["eager"] += 1
                self._zero_grad(opt)
                with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None, cache_enabled=False):
                    logits = self.net(*xs)
                loss = make_loss(logits, *targets)
                self._scaled(loss).backward()
                self._allreduce_grads()
                self._opt_step(opt)
                return loss.detach(), logits.detach()
            st["xs"] = [t.clone() for t in xs]
            st["targets"] = [t.clone() for t in targets]
            if self._flat is None:
                # no gradient tensors during the capture: the backward pass then WRITES every gradient into a tensor of this
                # graph's pool instead of adding it to a zeroed one -- one small kernel per parameter (53 of them, 0.25 ms per
                # update in profiles/r03_stats_sgan.txt) and the zeroing pass less.  Each head keeps its own gradient tensors.
                for q in self._params:
                    q.grad = None
            else:
                self._zero_grad(opt)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            # thread_local: the RCCL watchdog thread of a multi-rank job queries events while we capture; in the default
            # (global) mode that invalidates the capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype is not None, cache_enabled=False):
                    logits = self.net(*st["xs"])
                loss = make_loss(logits, *st["targets"])
                self._scaled(loss).backward()
            st["graph"], st["loss"], st["logits"] = g, loss, logits
            st["grads"] = [q.grad for q in self._params] if self._flat is None else None
            # the capture itself does not run the kernels: fall through to the first replay
        for dst, src in zip(st["xs"], xs):
            dst.copy_(src)
        for dst, src in zip(st["targets"], targets):
            dst.copy_(src)
        if st["grads"] is None:
            self._zero_grad(opt)
        st["graph"].replay()
        if st["grads"] is not None:
            for q, gr in zip(self._params, st["grads"]):       # this head's gradients (the other head's graph owns other tensors)
                q.grad = gr
        self._allreduce_grads()
        self._opt_step(opt)
        return st["loss"].detach(), st["logits"].detach()

    def _tuned(self, fn, *args):
        """``fn(*args)`` with MIOpen's timed solver search on while this trainer runs its convolutions (``tune_convolutions``),
        the process-wide flag put back afterwards."""
        if not self._tune:
            return fn(*args)
        import torch
        prev = torch.backends.cudnn.benchmark
        torch.backends.cudnn.benchmark = True
        try:
            return fn(*args)
        finally:
            torch.backends.cudnn.benchmark = prev

    def _graph_step(self, head, opt, make_loss, x, targets):
        return self._tuned(self._graph_step_impl, head, opt, make_loss, x, targets)

    def _step(self, opt, loss_fn, x):
        return self._tuned(self._step_impl, opt, loss_fn, x)

    def _inputs(self, x):
        return [to_nchw(a, self.device) for a in x]

    def _step_impl(self, opt, loss_fn, x):
        import torch
        self.net.train()
        if self._flat is not None:
            self._zero_grad(opt)
        else:
            opt.zero_grad(set_to_none=True)
        xs = self._inputs(x)
        if self.amp_dtype is not None:
            with torch.autocast("cuda", dtype=self.amp_dtype):
                logits = self.net(*xs)
        else:
            logits = self.net(*xs)
        loss = loss_fn(logits)
        self._scaled(loss).backward()
        self._allreduce_grads()
        self._opt_step(opt)
        return loss.detach(), logits.detach()

    def train_on_batch_c(self, x, y, sync=True):
        """c_model.train_on_batch([xz,yz,xy], y) -> (loss, accuracy) as Python floats (Keras), or as 0-d CUDA tensors
        with ``sync=False`` (no host synchronisation: the next step's launches overlap this step's kernels)."""
        import torch
        yt = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y).to(self.device).long().reshape(-1)
        if self.use_graph:
            loss, logits = self._graph_step("c", self.opt_c, lambda lg, t: c_loss(lg, t), x, (yt,))
        else:
            loss, logits = self._step(self.opt_c, lambda lg: c_loss(lg, yt), x)
        acc = (logits.argmax(dim=-1) == yt).float().mean()
        return (float(loss), float(acc)) if sync else (loss, acc)

    def train_on_batch_d(self, x, y, sample_weight=None, sync=True, class_weight=None):
        """d_model.train_on_batch([xz,yz,xy], y[, class_weight=w_classes]) -> loss (float, or a 0-d CUDA tensor with
        ``sync=False``).  ``class_weight`` (sgan.py:529-530) becomes a per-sample weight the way Keras does it
        (:func:`class_weight_to_sample_weight`)."""
        import torch
        if class_weight is not None:
            if sample_weight is not None:
                raise ValueError("give class_weight or sample_weight, not both")
            sample_weight = class_weight_to_sample_weight(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y, class_weight)
        yt = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y).to(self.device).float()
        sw = None if sample_weight is None else (sample_weight if isinstance(sample_weight, torch.Tensor)
                                                 else torch.as_tensor(np.asarray(sample_weight))).to(self.device)
        if self.use_graph:
            tg = (yt,) if sw is None else (yt, sw.float())
            loss, _ = self._graph_step("d" if sw is None else "dw", self.opt_d,
                                       (lambda lg, t: d_loss(lg, t)) if sw is None else (lambda lg, t, w_: d_loss(lg, t, w_)), x, tg)
        else:
            loss, _ = self._step(self.opt_d, lambda lg: d_loss(lg, yt, sw), x)
        return float(loss) if sync else loss

    def predict(self, x, batch_size=4096, fused=False):
        """c_model.predict: softmax class probabilities, float32 numpy.  ``fused=True``: the planes go through
        ``Discriminator.forward_fused`` (csrc/sgan_infer.hip, bf16 on the matrix cores with the BatchNorm layers folded in) instead
        of the PyTorch layers under this trainer's autocast; planes that chain does not take raise."""
        import torch
        self.model.eval()
        outs = []
        if fused:
            H, W = (int(v) for v in self._inputs([x[0][:1]])[0].shape[-2:]) if len(x[0]) else self.model.shapes[0][:2]
            if not self.model.fused_supported(H, W):
                raise ValueError("predict(fused=True): the fused SGAN trunk does not take %dx%d planes on this model (height and "
                                 "width multiples of 8, width <= 128, the model's own plane size)" % (H, W))
            for s in range(0, len(x[0]), batch_size):
                outs.append(self.model.forward_fused(*self._inputs([a[s:s + batch_size] for a in x])).cpu())
            return torch.cat(outs).numpy() if outs else np.zeros((0, self.model.n_classes), np.float32)
        with torch.no_grad():
            for s in range(0, len(x[0]), batch_size):
                xs = self._inputs([a[s:s + batch_size] for a in x])
                if self.amp_dtype is not None:
                    with torch.autocast("cuda", dtype=self.amp_dtype):
                        lg = self.model(*xs)
                else:
                    lg = self.model(*xs)
                outs.append(torch.softmax(lg.float(), dim=-1).cpu())
        return torch.cat(outs).numpy()


def _evaluate_c(trainer, x, y, batch_size=4096, fused=False):
    """c_model.evaluate([xz, yz, xy], y) (sgan.py:491: ``_, acc = c_model.evaluate(...)``): (sparse categorical
    cross-entropy, accuracy) over all samples, inference mode (BatchNorm moving statistics, no dropout).  ``fused``: as ``predict``."""
    p = trainer.predict(x, batch_size=batch_size, fused=fused).astype(np.float64)
    yi = np.asarray(y).reshape(-1).astype(np.int64)
    if len(yi) != len(p):
        raise ValueError("evaluate: %d label(s) for %d sample(s)" % (len(yi), len(p)))
    if len(yi) == 0:
        return 0.0, 0.0
    pt = np.clip(p[np.arange(len(yi)), yi], 1e-7, 1.0 - 1e-7)
    return float(-np.log(pt).mean()), float((p.argmax(axis=1) == yi).mean())


DiscriminatorTrainer.evaluate = _evaluate_c


def define_discriminator(xz_shape=(128, 128, 1), yz_shape=(128, 128, 1), xy_shape=(128, 128, 1), n_classes=3, device=None,
                         convolutions="library"):
    """Counterpart of sgan.define_discriminator (sgan.py:160): one shared trunk; the d / c heads are the two
    losses of :class:`DiscriminatorTrainer`.  ``convolutions``: the model's ``conv_impl`` ("library" or "hip", see the trainer)."""
    import torch
    if convolutions not in ("library", "hip"):
        raise ValueError("convolutions must be 'library' or 'hip', got %r" % (convolutions,))
    dev = torch.device(device) if device is not None else (
        torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    model = Discriminator([xz_shape, yz_shape, xy_shape], n_classes).to(dev).to(memory_format=torch.channels_last)
    model.conv_impl = convolutions
    return model


# ---- generator (sgan.py:57-122) ------------------------------------------------------------------------------------------

class Generator(_nn().Module):
    """g_model of sgan.py:57-122: three independent branches on one latent input (n, latent_dim); a branch is
    Dense(base*base*channels) -> ReLU -> Reshape (base, base, channels) [NHWC: unit j = (h*base + w)*channels + c] ->
    n_up x [Conv2DTranspose(channels, 4x4, stride 2, 'same') + BatchNormalization + ReLU] -> Conv2D(1, 7x7, 'same', tanh).
    ``forward`` returns three (n, 1, S, S) float32 tensors, S = base * 2**n_up (128 at the default size).

    Keras semantics.  The Dense stays in Keras order and its (n, base, base, channels) result is taken as the channels_last
    storage of an (n, channels, base, base) tensor (a view).  Conv2DTranspose 'same' with stride 2 and kernel 4 is the input
    gradient of a stride-2 4x4 'same' convolution, which TensorFlow pads 1 before and 1 after:
    out[oy, ox, co] = b[co] + sum in[iy, ix, ci] K[ky, kx, co, ci] over oy = 2 iy + ky - 1, ox = 2 ix + kx - 1, i.e.
    torch's ConvTranspose2d(k 4, s 2, padding 1) with weight[ci, co, ky, kx] = K[ky, kx, co, ci] and no flip.  The output
    convolution pads 3 on every side.  RandomNormal(0, 0.02) kernels, zero biases, BatchNorm momentum 0.99 (torch 0.01), eps 1e-3.

    In training mode batch norm cancels the bias of the transposed convolution in front of it, so the bias is not added (its
    gradient is exactly zero and none is handed back: the optimizer leaves it alone) and the moving mean is corrected by
    momentum * bias, which keeps inference -- where the bias is added -- in step."""

    def __init__(self, latent_dim=100, channels=128, base=8, n_up=4):
        nn = _nn()
        super().__init__()
        self.latent_dim, self.channels, self.base, self.n_up = int(latent_dim), int(channels), int(base), int(n_up)
        self.size = self.base * 2 ** self.n_up
        self.branches = nn.ModuleList()
        for _ in range(3):
            br = nn.Module()
            br.dense = nn.Linear(self.latent_dim, self.base * self.base * self.channels)
            br.ups = nn.ModuleList([nn.ConvTranspose2d(self.channels, self.channels, 4, stride=2, padding=1) for _ in range(self.n_up)])
            br.bns = nn.ModuleList([nn.BatchNorm2d(self.channels, eps=1e-3, momentum=0.01) for _ in range(self.n_up)])
            br.out = nn.Conv2d(self.channels, 1, 7, padding=3)
            self.branches.append(br)
        self._packs = {}                            # name -> (key of the tensors it was made from, value): generator_packs
        # the transposed convolutions in training mode: "library" (F.conv_transpose2d, i.e. MIOpen) or "hip" (nn_common.convt4s2:
        # csrc/convt_train.hip, forward and both gradients; reproducible bit for bit).  Inference and forward_fused never read it
        self.conv_impl = "library"
        for mod in self.modules():
            if isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
                nn.init.normal_(mod.weight, 0.0, 0.02)      # RandomNormal(stddev=0.02), sgan.py:60
                nn.init.zeros_(mod.bias)

    def _branch(self, z, br, adt):
        import torch
        import torch.nn.functional as F
        from .nn_common import bn_lrelu_pad, conv7_tanh, conv7_tanh_fused, convt4s2
        n = z.shape[0]
        h = F.relu(br.dense(z)).reshape(n, self.base, self.base, self.channels).permute(0, 3, 1, 2)      # NHWC storage, no copy
        fused = _FUSED_LAYERS and z.is_cuda and self.training and adt in (torch.float16, torch.bfloat16)
        for up, bn in zip(br.ups, br.bns):
            if not self.training:
                h = F.relu(bn(up(h)))
                continue
            if getattr(self, "conv_impl", "library") == "hip":      # a model pickled before the attribute existed: the library
                # the float32 master weight gets its gradient through the cast to the activations' (autocast) type
                zt = convt4s2(h, up.weight.to(h.dtype))
            else:
                zt = F.conv_transpose2d(h, up.weight, None, stride=2, padding=1)
            if fused:
                h = bn_lrelu_pad(zt, bn, slope=0.0, pad=0, conv_bias=up.bias)
            else:
                if bn.track_running_stats and bn.momentum is not None:
                    # the statistics are those of conv(x) + bias, whose mean is larger by exactly the bias: new = (1 - m) old + m (mean + b).
                    # Applied to the old value, in front of the layer (autograd keeps the buffer the layer saw)
                    m = float(bn.momentum)
                    with torch.no_grad():
                        bn.running_mean.add_(up.bias.detach().to(bn.running_mean.dtype), alpha=m / (1.0 - m))
                h = F.relu(bn(zt))
        if fused and conv7_tanh_fused(h, br.out):
            return conv7_tanh(h, br.out)
        return torch.tanh(br.out(h)).float() if h.dtype in (torch.float16, torch.bfloat16) else torch.tanh(br.out(h))

    def forward(self, z):
        """[xz, yz, xy] images in [-1, 1], each (n, 1, S, S)."""
        import torch
        adt = torch.get_autocast_dtype("cuda") if (z.is_cuda and torch.is_autocast_enabled("cuda")) else None
        return [self._branch(z, br, adt) for br in self.branches]

    # ---- inference on the fused HIP chain (csrc/gen_infer.hip + the forward of csrc/gen.hip) -------------------------------
    def packs_key(self):
        """What :func:`generator_packs` is cached on: the version counter and the storage of every parameter AND every BatchNorm
        buffer.  An eager optimizer step, ``DeviceAdam`` (it increments the versions of what it wrote through raw pointers),
        ``set_keras_weights``, ``load_state_dict`` and ``.to()`` change it; so does a training-mode forward, the fused one too: its
        kernel advances the moving statistics through raw pointers, but ``nn_common._bn_side_effects`` then writes
        ``num_batches_tracked`` and ``running_mean`` with ordinary in-place ops, and both are read here."""
        return tuple((t._version, t.data_ptr()) for t in list(self.parameters()) + list(self.buffers()))

    def generator_packs(self, dtype=None):
        """:func:`generator_packs` of this model, cached until :meth:`packs_key` changes (one entry per dtype)."""
        import torch
        dtype = torch.bfloat16 if dtype is None else dtype
        key = self.packs_key()
        hit = self._packs.get(dtype)
        if hit is None or hit[0] != key:
            hit = self._packs[dtype] = (key, generator_packs(self, dtype, cached=False))
        return hit[1]

    def fused_supported(self):
        """True when the fused inference chain takes this model's geometry: 128 channels, every transposed convolution on a plane
        whose edge is a multiple of 8 in [8, 128] (``rml_gen_up_supported``), images of at most 256 x 256."""
        from . import _lib
        lib = _lib.load()
        return (len(self.branches) == 3 and all(bool(lib.rml_gen_up_supported(self.base << l, self.base << l, self.channels)) for l in range(self.n_up))
                and int(lib.rml_sgan_generate_workspace_bytes(1, self.base, self.n_up, self.channels)) > 0)

    def forward_fused(self, z, dtype=None):
        """``g_model.predict(z)`` on the fused HIP chain: three (n, 1, S, S) float32 CUDA tensors in [-1, 1] from (n, latent_dim)
        latent points, in inference mode whatever ``self.training`` says (moving statistics; the BatchNorm layers folded into the
        transposed convolutions, :func:`fold_generator`).  ``dtype``: the operand type of the matrix cores, bfloat16 (default) or
        float16.  A sample's images do not depend on the batch around it.  Raises ValueError for a geometry the chain does not take
        (there is no fall-back), for a model that is not on a GPU, and when ``z`` asks for a gradient."""
        import torch
        from . import _lib
        dtype = torch.bfloat16 if dtype is None else dtype
        par = next(self.parameters())
        if par.device.type != "cuda":
            raise ValueError("forward_fused runs on the GPU: move the generator to a CUDA device (there is no CPU path)")
        if dtype not in (torch.bfloat16, torch.float16) or par.dtype != torch.float32:
            raise ValueError("forward_fused: bfloat16 or float16 operands from a float32 model expected")
        if isinstance(z, torch.Tensor) and z.requires_grad and torch.is_grad_enabled():
            raise ValueError("forward_fused is inference only: it has no backward (z requires a gradient)")
        if not self.fused_supported():
            raise ValueError("the fused generator chain takes 128 channels and transposed convolutions on planes whose edge is a multiple "
                             "of 8 in [8, 128]: got channels=%d, base=%d, n_up=%d" % (self.channels, self.base, self.n_up))
        dev = par.device
        with torch.no_grad():
            zt = (z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z))).to(device=dev, dtype=torch.float32)
            if zt.ndim != 2 or zt.shape[1] != self.latent_dim:
                raise ValueError("forward_fused: (n, %d) latent points expected, got %s" % (self.latent_dim, tuple(zt.shape)))
            zt = zt.contiguous()
            n, S = int(zt.shape[0]), self.size
            outs = [torch.empty((n, 1, S, S), dtype=torch.float32, device=dev) for _ in range(3)]
            if n == 0:
                return outs
            lib = _lib.load()
            pk = self.generator_packs(dtype)
            nbytes = int(lib.rml_sgan_generate_workspace_bytes(n, self.base, self.n_up, self.channels))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.rml_sgan_generate(_lib.context(dev), _lib.ptr(zt), n, self.latent_dim, self.base, self.n_up, self.channels,
                                                 1 if dtype == torch.bfloat16 else 0, _lib.ptr(pk["dense_w"]), _lib.ptr(pk["dense_b"]),
                                                 _lib.ptr(pk["up_wt"]), _lib.ptr(pk["up_bias"]), _lib.ptr(pk["out_w"]), _lib.ptr(pk["out_b"]),
                                                 _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(ws), nbytes,
                                                 _lib.stream_ptr(dev)), "rml_sgan_generate")
        return outs

    def predict(self, z, batch_size=256, return_numpy=True, amp_dtype=None, fused=False):
        """``g_model.predict(z)`` (sgan.py:450): inference mode (moving statistics), a list of three (n, S, S, 1) float32 arrays
        in [-1, 1]; with ``return_numpy=False`` three (n, 1, S, S) float32 tensors on the model's device, which
        ``DiscriminatorTrainer.train_on_batch_d`` takes without a host trip.  ``amp_dtype``: run the layers under autocast.
        ``fused=True``: the images come from :meth:`forward_fused` (csrc/gen_infer.hip) with ``amp_dtype`` as the operand type,
        bfloat16 when none is given; a model that chain does not take raises ValueError."""
        import torch
        if fused:
            cat = self.forward_fused(z, dtype=amp_dtype)
            if not return_numpy:
                return cat
            return [c.permute(0, 2, 3, 1).contiguous().cpu().numpy() for c in cat]
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        zt = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z))
        zt = zt.to(device=dev, dtype=dt)
        was_training = self.training
        self.eval()
        outs = [[], [], []]
        try:
            with torch.no_grad():
                for s in range(0, zt.shape[0], batch_size):
                    if amp_dtype is not None and dev.type == "cuda":
                        with torch.autocast("cuda", dtype=amp_dtype):
                            imgs = self(zt[s:s + batch_size])
                    else:
                        imgs = self(zt[s:s + batch_size])
                    for o, im in zip(outs, imgs):
                        o.append(im.float())
        finally:
            self.train(was_training)
        cat = [torch.cat(o) if o else torch.zeros((0, 1, self.size, self.size), device=dev) for o in outs]
        if not return_numpy:
            return [c.contiguous() for c in cat]
        return [c.permute(0, 2, 3, 1).contiguous().cpu().numpy() for c in cat]

    # ---- Keras layout in / out -------------------------------------------------------------------------
    def keras_weights(self):
        """Parameters and moving statistics in Keras layouts, float64 numpy; per branch
        ``[(dense kernel (latent, base*base*channels), bias), [(ConvT kernel (4, 4, out, in), bias, gamma, beta, moving_mean,
        moving_variance)] x n_up, (output kernel (7, 7, channels, 1), bias)]``."""
        def a(t):
            return t.detach().double().cpu().numpy()
        out = []
        for br in self.branches:
            ups = [(a(up.weight.permute(2, 3, 1, 0)), a(up.bias), a(bn.weight), a(bn.bias), a(bn.running_mean), a(bn.running_var))
                   for up, bn in zip(br.ups, br.bns)]
            out.append([(a(br.dense.weight.t()), a(br.dense.bias)), ups, (a(br.out.weight.permute(2, 3, 1, 0)), a(br.out.bias))])
        return out

    def set_keras_weights(self, branches):
        """Inverse of :meth:`keras_weights` (what ``layer.get_weights()`` of a trained ``g_model_XXXX.h5`` holds, sgan.py:496-497)."""
        import torch
        if len(branches) != len(self.branches):
            raise ValueError("expected %d branches" % len(self.branches))

        def put(dst, arr, what):
            t = torch.as_tensor(np.asarray(arr), dtype=dst.dtype)
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError("%s: Keras array gives %s, the layer holds %s" % (what, tuple(t.shape), tuple(dst.shape)))
            dst.copy_(t.to(dst.device))

        with torch.no_grad():
            for bi, (br, (dense, ups, outc)) in enumerate(zip(self.branches, branches)):
                if len(ups) != len(br.ups):
                    raise ValueError("branch %d: expected %d (transposed convolution + batch-norm) tuples" % (bi, len(br.ups)))
                put(br.dense.weight, np.asarray(dense[0]).T, "branch %d dense kernel" % bi)
                put(br.dense.bias, dense[1], "branch %d dense bias" % bi)
                for li, (up, bn, (k, b, g, be, mu, var)) in enumerate(zip(br.ups, br.bns, ups)):
                    what = "branch %d layer %d" % (bi, li)
                    put(up.weight, np.asarray(k).transpose(3, 2, 0, 1), what + " kernel")
                    put(up.bias, b, what + " bias")
                    put(bn.weight, g, what + " gamma"); put(bn.bias, be, what + " beta")
                    put(bn.running_mean, mu, what + " moving_mean"); put(bn.running_var, var, what + " moving_variance")
                put(br.out.weight, np.asarray(outc[0]).transpose(3, 2, 0, 1), "branch %d output kernel" % bi)
                put(br.out.bias, outc[1], "branch %d output bias" % bi)
        return self


def define_generator(latent_dim=100, device=None, convolutions="library"):
    """Counterpart of sgan.define_generator (sgan.py:90-122): the model on the device, channels_last.  ``convolutions``: the model's
    ``conv_impl`` ("library" or "hip", see :class:`GanTrainer`)."""
    import torch
    if convolutions not in ("library", "hip"):
        raise ValueError("convolutions must be 'library' or 'hip', got %r" % (convolutions,))
    dev = torch.device(device) if device is not None else (
        torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    model = Generator(latent_dim=latent_dim).to(dev).to(memory_format=torch.channels_last)
    model.conv_impl = convolutions
    return model


def fold_generator(model):
    """The inference-mode generator with every BatchNorm folded into the transposed convolution in front of it (as
    :func:`fold_batchnorm` does for the classifier), float64 on the model's device, in Keras layouts.  Per branch
    ``[(dense kernel (latent, base*base*channels), bias), [(w' (4, 4, out, in), b')] x n_up, (output kernel (7, 7, channels, 1), bias)]``
    with ``s = gamma / sqrt(moving_variance + eps)``, ``w'[ky, kx, co, ci] = K[ky, kx, co, ci] * s[co]`` and
    ``b' = beta + (bias - moving_mean) * s``; a layer is then ``relu(conv_transpose(x, w') + b')``."""
    def d(t):
        return t.detach().double()
    out = []
    for br in model.branches:
        ups = []
        for up, bn in zip(br.ups, br.bns):
            sc = d(bn.weight) / (d(bn.running_var) + float(bn.eps)).sqrt()
            ups.append((d(up.weight).permute(2, 3, 1, 0) * sc.reshape(1, 1, -1, 1), d(bn.bias) + (d(up.bias) - d(bn.running_mean)) * sc))
        out.append([(d(br.dense.weight).t(), d(br.dense.bias)), ups, (d(br.out.weight).permute(2, 3, 1, 0), d(br.out.bias))])
    return out


def pack_up_kernel(w):
    """A folded transposed-convolution kernel (4, 4, out, in) in the layout of ``rml_gen_up_forward``: (4, out, 4 * in) with
    ``wt[p*2+q, co, (a*2+b)*in + ci] = w[3-p-2a, 3-q-2b, co, ci]`` -- per output phase (p, q) the four taps its 2x2 input window
    meets, window row a / column b major."""
    import torch
    return torch.stack([torch.cat([w[3 - p - 2 * a, 3 - q - 2 * b] for a in (0, 1) for b in (0, 1)], dim=1)
                        for p in (0, 1) for q in (0, 1)])


def generator_packs(model, dtype=None, cached=True):
    """:func:`fold_generator` in the layouts of ``rml_sgan_generate``, computed in float64 and cast once, on the model's device (CPU
    tensors for a CPU model): ``dense_w`` (3, latent, base*base*channels) and ``dense_b`` float32; ``up_wt`` (3, n_up, 4, channels,
    4*channels) of ``dtype`` (bfloat16 unless given; :func:`pack_up_kernel`) and ``up_bias`` (3, n_up, channels) float32; ``out_w``
    (3, 49, channels) and ``out_b`` (3,) float32.  With ``dtype=torch.float64`` every array stays float64 (what the tests' NumPy twin
    reads).  ``cached``: kept on the model until one of its parameters or BatchNorm buffers is written (``Generator.packs_key``)."""
    import torch
    dtype = torch.bfloat16 if dtype is None else dtype
    if cached:
        return model.generator_packs(dtype)
    f = fold_generator(model)
    fdt = torch.float64 if dtype == torch.float64 else torch.float32
    C, dev = model.channels, next(model.parameters()).device
    up_wt = [torch.stack([pack_up_kernel(w) for w, _ in ups]) if ups else torch.zeros((0, 4, C, 4 * C), dtype=torch.float64, device=dev)
             for _, ups, _ in f]
    up_b = [torch.stack([b for _, b in ups]) if ups else torch.zeros((0, C), dtype=torch.float64, device=dev) for _, ups, _ in f]
    return {"dense_w": torch.stack([dn[0] for dn, _, _ in f]).to(fdt).contiguous(),
            "dense_b": torch.stack([dn[1] for dn, _, _ in f]).to(fdt).contiguous(),
            "up_wt": torch.stack(up_wt).to(dtype).contiguous(), "up_bias": torch.stack(up_b).to(fdt).contiguous(),
            "out_w": torch.stack([o[0].reshape(49, C) for _, _, o in f]).to(fdt).contiguous(),
            "out_b": torch.stack([o[1].reshape(()) for _, _, o in f]).to(fdt).contiguous()}


class GanTrainer:
    """``define_gan`` +``gan_model.train_on_batch`` (sgan.py:220-235, 534-537): the loss is ``d_loss(D(G(z)), y)``.
    ``define_gan`` freezes every discriminator layer except BatchNormalization, so this optimizer -- its own
    Adam(2e-4, beta1 0.5, eps 1e-7) -- updates all generator parameters and the discriminator's BatchNorm gammas and betas
    (1 600 values at the default size).  During the step the discriminator runs in training mode (batch statistics, moving
    statistics and counters advance, dropout active); its other weights get no gradient at all (``torch.autograd.grad`` over the
    trained parameters only: the weight-gradient convolutions are skipped) and nothing is frozen afterwards.  The loss scale is the
    discriminator trainer's.  ``.grad`` is never touched, so a trainer with captured heads keeps its gradient tensors."""

    def __init__(self, generator, disc_trainer, lr=2e-4, beta1=0.5, convolutions=None):
        """``convolutions``: None (default) leaves ``generator.conv_impl`` as it is; "library" runs the generator's transposed
        convolutions in training mode through ``F.conv_transpose2d``; "hip" runs them and their gradients on csrc/convt_train.hip
        (nn_common.convt4s2): no convolution library, no workspace zeroing, every gradient the same bits on every call.  With a
        discriminator trainer that also uses ``convolutions="hip"`` the g update then runs no library convolution at all."""
        import torch
        import torch.distributed as dist
        nn = _nn()
        if convolutions not in (None, "library", "hip"):
            raise ValueError("convolutions must be None, 'library' or 'hip', got %r" % (convolutions,))
        if convolutions is not None:
            generator.conv_impl = convolutions
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("GanTrainer: data parallelism of the generator step is not implemented")
        self.generator, self.disc_trainer, self.disc = generator, disc_trainer, disc_trainer.model
        self.device = disc_trainer.device
        if next(generator.parameters()).device != self.device:
            raise ValueError("GanTrainer: generator and discriminator live on different devices")
        self.bn_params = [p for m in self.disc.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)) for p in (m.weight, m.bias)]
        self.params = [p for p in generator.parameters() if p.requires_grad] + self.bn_params
        ids = {id(p): k for k, p in self.disc.named_parameters()}
        self.param_names = ["g." + k for k, p in generator.named_parameters() if p.requires_grad] + ["d." + ids[id(p)] for p in self.bn_params]
        self.opt = torch.optim.Adam(self.params, lr=lr, betas=(beta1, 0.999), eps=1e-7, fused=self.device.type == "cuda")
        self._dev_adam = None
        if disc_trainer._dev_adam is not None:
            from .nn_common import DeviceAdam
            shared = next(iter(disc_trainer._dev_adam.values())).state
            self._dev_adam = DeviceAdam(self.params, lr, (beta1, 0.999), 1e-7, scale=disc_trainer._scale_t, scaler_state=shared, mirror=self.opt)

    def _loss(self, z, y):
        import torch
        dt = self.disc_trainer
        self.generator.train()
        self.disc.train()
        zt = (z if isinstance(z, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(z))).to(
            device=self.device, dtype=next(self.generator.parameters()).dtype)
        yt = (y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))).to(self.device).float()
        if dt.amp_dtype is not None:
            with torch.autocast("cuda", dtype=dt.amp_dtype):
                logits = self.disc(*self.generator(zt))
        else:
            logits = self.disc(*self.generator(zt))
        return d_loss(logits, yt)

    def gradients(self, z, y):
        """(loss, gradients of the SCALED loss for ``self.params``, None where a parameter takes no part) without an update."""
        import torch
        loss = self._loss(z, y)
        grads = list(torch.autograd.grad(self.disc_trainer._scaled(loss), self.params, allow_unused=True))
        for i, (p, g) in enumerate(zip(self.params, grads)):
            # laid out like the parameter (channels_last kernels), as the accumulation into .grad would have done: the fused Adam
            # runs over the storage order
            if g is not None and (g.stride() != p.stride() or g.dtype != p.dtype):
                grads[i] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
        return loss.detach(), grads

    def train_on_batch_g(self, z, y, sync=True):
        """gan_model.train_on_batch(z, y) -> loss (float, or a 0-d tensor with ``sync=False``); ``y``: the smoothed positives."""
        loss, grads = self.disc_trainer._tuned(self.gradients, z, y)
        if self._dev_adam is not None:
            self._dev_adam.step(grads)
        else:
            # torch's optimizers read .grad: lend it the gradients for the update and hand back what was there
            kept = [p.grad for p in self.params]
            try:
                for p, g in zip(self.params, grads):
                    p.grad = g
                self.disc_trainer.scaler.step(self.opt)
                self.disc_trainer.scaler.update()
            finally:
                for p, g in zip(self.params, kept):
                    p.grad = g
        return float(loss) if sync else loss


# ---- fake samples, the data product, the loop (sgan.py:396-543) ----------------------------------------------------------

def smooth_positive_labels(y, rng):
    """class 1 -> [0.7, 1.2) (sgan.py:396-398)"""
    return y - 0.3 + rng.random(y.shape) * 0.5


def smooth_negative_labels(y, rng):
    """class 0 -> [0, 0.3) (sgan.py:401-403)"""
    return y + rng.random(y.shape) * 0.3


def generate_latent_points(latent_dim, n, rng):
    """sgan.py:439-442: (n, latent_dim) standard normal points."""
    return rng.standard_normal(size=(n, latent_dim))


def generate_fake_samples(generator, latent_dim, n, rng, return_numpy=True, amp_dtype=None, fused=False):
    """sgan.py:445-454: ``generator.predict`` on n latent points, and their labels in [0, 0.3).  ``fused``: as ``Generator.predict``
    (the draws from ``rng`` are the same numbers in the same order either way)."""
    z = generate_latent_points(latent_dim, n, rng)
    if fused:
        images = generator.predict(z, return_numpy=return_numpy, amp_dtype=amp_dtype, fused=True)
    else:
        images = generator.predict(z, return_numpy=return_numpy, amp_dtype=amp_dtype)
    return images, smooth_negative_labels(np.zeros((n, 1)), rng)


def arena_planes(images, sizes=(XZ_SIZE, YZ_SIZE, XY_SIZE)):
    """Three (n, 1, S, S) image tensors in [-1, 1] -> three (n, rows, cols) float32 numpy arrays at the radar arena
    (sgan.py:466-481): RADAR_MAX * (v + 1) / 2, then Pillow's BICUBIC (csrc/resize.hip, bit-identical to Pillow); ``sizes`` in
    Pillow's (cols, rows) order."""
    from .common import RADAR_MAX
    from .nn_common import resize_bicubic
    planes = []
    for v, (cols, rows) in zip(images, sizes):
        p = (float(RADAR_MAX) * (v[:, 0] + 1.0) / 2.0).contiguous()
        planes.append(resize_bicubic(p, (int(rows), int(cols)), scale=False).cpu().numpy())
    return planes


def generated_samples(generator, latent_dim, n, rng, sizes=(XZ_SIZE, YZ_SIZE, XY_SIZE), fused=False):
    """The samples of ``summarize_performance`` (sgan.py:462-483): n fake images scaled to RADAR_MAX * (v + 1) / 2 and resized back
    to the radar arena with Pillow's BICUBIC (csrc/resize.hip, bit-identical to Pillow); ``sizes`` in Pillow's (cols, rows) order.
    Returns a list of (xz, yz, xy) float32 tuples.  ``fused``: as ``Generator.predict``."""
    if fused:
        fake, _ = generate_fake_samples(generator, latent_dim, n, rng, return_numpy=False, fused=True)
    else:
        fake, _ = generate_fake_samples(generator, latent_dim, n, rng, return_numpy=False)
    planes = arena_planes(fake, sizes)
    return [(planes[0][i], planes[1][i], planes[2][i]) for i in range(n)]


def generate_dataset(generator, n, latent_dim=100, rng=None, sizes=(XZ_SIZE, YZ_SIZE, XY_SIZE), batch_size=4096, path=None, fused=True):
    """The generator's data product (``generated_data_XXXX.pickle``, sgan.py:462-488) at any n, in batches of ``batch_size``: per
    batch the latent points (``rng``, this module's unless given), the images (``Generator.predict``; ``fused``: on the HIP chain
    of csrc/gen_infer.hip), RADAR_MAX * (v + 1) / 2 and the Pillow-exact resize back to the arena (:func:`arena_planes`).  Returns
    the list of (xz, yz, xy) float32 tuples, or -- with ``path`` -- writes :func:`save_generated`'s pickle and returns the number of
    samples in it."""
    rng = _rng(rng)
    bs = max(1, int(batch_size))
    samples = []
    for s in range(0, int(n), bs):
        nb = min(bs, int(n) - s)
        z = generate_latent_points(latent_dim, nb, rng)
        planes = arena_planes(generator.predict(z, return_numpy=False, fused=bool(fused)), sizes)
        samples += [(planes[0][i], planes[1][i], planes[2][i]) for i in range(nb)]
    if path is not None:
        return save_generated(path, samples)
    return samples


def save_generated(path, samples):
    """``generated_data_XXXX.pickle`` (sgan.py:483-488): the data-set format of datasets.py with every label 'generated_data'."""
    data = {"samples": [tuple(np.asarray(p, np.float32) for p in s) for s in samples], "labels": ["generated_data"] * len(samples)}
    with open(path, "wb") as fp:
        pickle.dump(data, fp)
    return len(data["labels"])


def _flatten_weights(obj, prefix="w"):
    if isinstance(obj, (list, tuple)):
        out = {}
        for i, o in enumerate(obj):
            out.update(_flatten_weights(o, "%s_%d" % (prefix, i)))
        return out
    return {prefix: np.asarray(obj)}


def save_model_npz(path, model):
    """``model.keras_weights()`` as an ``.npz`` (keys w_<index path>): the stand-in for the reference's ``.h5`` files."""
    np.savez(path, **_flatten_weights(model.keras_weights()))


def _rng(given):
    return given if given is not None else rng


def augment_data(x, rotation_range=1.0, zoom_range=0.3, noise_sd=1.0, rng=None, device=None):
    """``augment_data`` of sgan.py:238-326, the function of dnn.py:94-182: see ``radar_ml_amd.dnn.augment_data``.  The noise comes from
    this module's ``rng`` (``default_rng(1234)``) unless ``rng`` is given."""
    return prep.augment_data(x, rotation_range, zoom_range, noise_sd, _rng(rng), device)


def balance_classes(data, labels, samples_sup, shuffle=True, rng=None):
    """``balance_classes`` of sgan.py:329-393: every class is upsampled to the size of the largest one -- per class, from the most common
    down, the rows ``sklearn.utils.resample(..., replace=True, random_state=1234)`` picks on the host -- and the result is shuffled with
    ``rng`` (this module's unless given).  ``data`` may be a CUDA tensor: the gather then runs on the device and the result stays there.
    Classes that are balanced already: the three inputs themselves are returned and nothing is drawn."""
    return prep.balance_classes(data, labels, samples_sup, shuffle, _rng(rng))


def preprocess_data(args, data, labels, samples_sup, *, rng=None, device=None, return_numpy=True):
    """``preprocess_data`` of sgan.py:617-727 with the arrays on the GPU: as ``radar_ml_amd.dnn.preprocess_data`` (same draws, same order,
    same launches) with a resize to 128 x 128, the supervised mask ``samples_sup`` carried through shuffle and split, and
    :func:`balance_classes` on the training part (its shuffle is the last use of ``rng``).  Returns ``train_set, val_set, n_classes,
    w_classes`` with ``train_set = (X, y, sup)`` balanced and ``val_set = (X_val, y_val)``, or -- the reference's rule for an empty
    validation set (``train_split`` 1.0) -- the training part as it was before balancing.  ``return_numpy=False`` leaves the ``X`` as CUDA
    tensors, which :func:`train` takes as they are.  Planes are handled in float32: integer / float64 planes are converted first."""
    return prep.preprocess_sgan(args, data, labels, samples_sup, RESCALE, _rng(rng), device, return_numpy)


def select_supervised_samples(dataset, rng, n_samples=150, n_classes=3):
    """sgan.py:406-422: a class-balanced supervised subset (drawn with replacement from the samples flagged ``sup``)."""
    X, y, sup = dataset
    y, sup = np.asarray(y), np.asarray(sup, dtype=bool)
    n_per_class = int(n_samples / n_classes)
    ix_all, y_all = [], []
    for c in range(n_classes):
        cand = np.nonzero((y == c) & sup)[0]
        if len(cand) == 0:
            raise ValueError("no supervised samples of class %d" % c)
        ix_all.append(cand[rng.integers(0, len(cand), n_per_class)])
        y_all += [c] * n_per_class
    return np.concatenate(ix_all), np.asarray(y_all)


def train(g_model, disc_trainer, gan, train_set, val_set, n_classes, w_classes=None, latent_dim=100, n_epochs=15, n_batch=32,
          results_dir=None, seed=1234, fused_generate=False):
    """The training loop of sgan.py:504-543: per step the four updates c, d on real samples, d on fake samples, g; per epoch the
    classifier's accuracy on ``val_set``, ``generated_data_%04d.pickle`` and the models (``.npz`` of ``keras_weights()``).
    ``train_set`` = (X (N, H, W, 3), y, sup), ``val_set`` = (X, y, ...).  The data set is uploaded once and batches are gathered
    on the device; every draw comes from one ``np.random.default_rng(seed)``.  ``fused_generate``: the fake samples of the third
    update and of the epoch's data product come from ``Generator.forward_fused`` (csrc/gen_infer.hip; same draws).  Returns the
    per-step (c_loss, c_acc, dr_loss, df_loss, g_loss)."""
    import torch
    rng = np.random.default_rng(seed)
    dev = disc_trainer.device
    # a CUDA tensor (preprocess_data(return_numpy=False)) stays on its device
    X = (train_set[0] if isinstance(train_set[0], torch.Tensor) else torch.as_tensor(np.asarray(train_set[0]))).to(device=dev, dtype=torch.float32)
    planes = [X[..., i].unsqueeze(1).contiguous() for i in range(3)]          # three (N, 1, H, W), resident
    sup_ix, y_sup = select_supervised_samples(train_set, rng, n_classes=n_classes)
    bat_per_epo = int(X.shape[0] / n_batch)
    n_steps = bat_per_epo * n_epochs
    half_batch = int(n_batch / 2)
    logger.info("Starting training loop.")
    logger.info("n_epochs=%d, n_batch=%d, 1/2=%d, b/e=%d, steps=%d" % (n_epochs, n_batch, half_batch, bat_per_epo, n_steps))

    def gather(ix):
        it = torch.as_tensor(ix, dtype=torch.long, device=dev)
        return [p.index_select(0, it) for p in planes]

    history = []
    for i in range(n_steps):
        ix = rng.integers(0, len(sup_ix), half_batch)
        c_l, c_acc = disc_trainer.train_on_batch_c(gather(sup_ix[ix]), y_sup[ix])
        ix = rng.integers(0, X.shape[0], half_batch)
        y_real = smooth_positive_labels(np.ones((half_batch, 1)), rng)
        dr_l = disc_trainer.train_on_batch_d(gather(ix), y_real, class_weight=w_classes)
        x_fake, y_fake = generate_fake_samples(g_model, latent_dim, half_batch, rng, return_numpy=False, amp_dtype=disc_trainer.amp_dtype,
                                               fused=bool(fused_generate))
        df_l = disc_trainer.train_on_batch_d(x_fake, y_fake)
        z = generate_latent_points(latent_dim, n_batch, rng)
        g_l = gan.train_on_batch_g(z, smooth_positive_labels(np.ones((n_batch, 1)), rng))
        logger.debug("Training results at step %d: c[%.3f,%.0f], d_r[%.3f], d_f[%.3f], g[%.3f]" % (i + 1, c_l, c_acc * 100, dr_l, df_l, g_l))
        history.append((c_l, c_acc, dr_l, df_l, g_l))
        if bat_per_epo and (i + 1) % bat_per_epo == 0:
            Xv = val_set[0] if isinstance(val_set[0], torch.Tensor) else np.asarray(val_set[0])
            _, acc = disc_trainer.evaluate([Xv[..., 0], Xv[..., 1], Xv[..., 2]], val_set[1])
            logger.info("Classifier accuracy at step %d: %.2f%%" % (i + 1, acc * 100))
            if results_dir is not None:
                f1 = os.path.join(results_dir, "generated_data_%04d.pickle" % (i + 1))
                f2 = os.path.join(results_dir, "g_model_%04d.npz" % (i + 1))
                f3 = os.path.join(results_dir, "c_model_%04d.npz" % (i + 1))
                save_generated(f1, generated_samples(g_model, latent_dim, 100, rng, fused=bool(fused_generate)))
                save_model_npz(f2, g_model)
                save_model_npz(f3, disc_trainer.model)
                logger.info("Saved: %s, %s, and %s" % (f1, f2, f3))
    return history
