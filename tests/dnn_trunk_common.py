"""Cases and references of the CNN trunk sweep (tests/test_dnn_trunk_cpu.py, tests/test_dnn_trunk_gpu.py).

csrc/dnn.hip serves rml_dnn_trunk with k_dnn_trunk_rf (conv1 image in registers; a workgroup or a wave per sample) and k_dnn_trunk (conv1
image in LDS; strips of SR = 4 / 2 / 1 conv2 rows, with or without the register prefetch of the next plane, float32 or bf16 planes).
rml_dnn_trunk_path -- the launchers' own predicates -- says which one a call takes; :func:`path` wraps it and SHAPES lists planes that
reach every combination it can report.

:func:`twin` is the reference: the two layers in float64 (or float32) torch on the CPU on the operands the kernels see -- planes, w1
and w2 rounded to bf16, the conv1 bias as float32 (rf) or one bf16 (LDS kernel), the conv1 image rounded to bf16 -- with TensorFlow's
bottom / right 'same' zeros.  Two operand families:

* exact integers (:func:`int_model`, :func:`int_planes`): every conv1 value is an integer of magnitude <= 256 (exact in bf16) and every
  conv2 partial sum an integer below 2^24 (exact in float32 in any order), so a correct kernel equals the twin BIT FOR BIT; the final
  bf16 rounding is a round-to-nearest-even of an exact integer, and between 256 and 512 the odd integers are exact ties;
  :func:`frac_model` adds k / 256 to the conv1 biases -- still exact everywhere, but only with every bit of the bias carried;
* real values (:func:`real_model`, :func:`real_planes`): the weights of tests/sgan_infer_common.make_model, planes uniform in [-1, 1]:
  roundings on load, bias precision, a truncating conversion -- held to half a bf16 ulp + 4 * E32, E32 being what another float32
  summation order costs, measured between the float32 and float64 twins."""
import collections
import functools
import importlib

import numpy as np

# (H, W, bf16 planes too, what the shape is for); rml_dnn_trunk_path is the authority on the path (test_dnn_trunk_cpu.py prints the table)
SHAPES = (
    (4, 4, False, "rf, one partial tile, the smallest plane"),
    (4, 8, True, "rf, one partial tile, the smallest bf16 plane"),
    (8, 8, True, "rf, one partial tile"),
    (24, 16, True, "rf, one partial tile of 24 pixels"),
    (44, 36, False, "rf, OW2 = 9, four tiles with the last partial"),
    (68, 72, True, "rf, OW2 = 18, 10 tiles: two waves of a split workgroup take a second tile, the pixel walk wraps rows"),
    (80, 80, True, "rf, the default plane"),
    (80, 88, True, "rf, the largest plane with W % 8 == 0"),
    (84, 84, False, "rf, the largest square"),
    (124, 64, True, "LDS SR=4 WPC=2, OH2 = 31: the last strip has 3 rows; prefetch for bf16 planes only"),
    (128, 64, True, "LDS SR=4, whole strips; 1024 bf16 quads: the last plane that prefetches"),
    (136, 64, True, "LDS SR=4, OH2 = 34: the last strip has 2 rows; no prefetch for either dtype"),
    (252, 32, True, "LDS SR=4, two of the five pixel tiles live; prefetch for bf16 planes"),
    (196, 36, False, "LDS SR=4, OH2 = 49: the last strip has 1 row; 1764 float32 quads: the one float32 corner that prefetches at SR=4"),
    (160, 80, True, "SR=4 fits one workgroup per CU but not two: SR=2"),
    (60, 128, True, "LDS SR=2, OH2 = 15: the last strip has 1 row; prefetch for bf16 planes"),
    (128, 128, True, "LDS SR=2, no prefetch"),
    (28, 248, True, "LDS SR=1, 12 conv1 tiles; prefetch for both dtypes"),
    (36, 256, True, "LDS SR=1, no prefetch"),
)
UNSUPPORTED = (40, 264)          # 13 conv1 tiles at SR=1: no kernel
DISTINCT = 7                     # large batches repeat this many distinct samples (row % DISTINCT)

Path = collections.namedtuple("Path", "kernel sr wpc prefetch split gx")
KERNEL_NAMES = {0: "unsupported", 1: "k_dnn_trunk_rf", 2: "k_dnn_trunk"}


def dnn_module():
    return importlib.import_module("radar_ml_amd.dnn")


def path(H, W, bf16, B=1, num_cu=256):
    """rml_dnn_trunk_path as a Path (host only: needs the library, no GPU)"""
    import ctypes
    from radar_ml_amd import _lib
    out = (ctypes.c_int * 6)()
    rc = _lib.load().rml_dnn_trunk_path(int(H), int(W), 1 if bf16 else 0, int(B), int(num_cu), ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, rc
    return Path(*[int(v) for v in out])


def combo(p):
    """what the coverage assertion counts: (kernel, SR, prefetch) -- the input dtype comes beside it"""
    return (p.kernel, p.sr, p.prefetch)


def cases():
    """(H, W, bf16) of every plane shape and input dtype of the sweep"""
    return [(H, W, bf) for (H, W, both, _) in SHAPES for bf in ((False, True) if both else (False,))]


def batches(H, W, bf16, num_cu, big=False):
    """the batch sizes of a case, from the query: around the split threshold of the rf kernel, past the grid of the LDS kernel"""
    p = path(H, W, bf16, 1, num_cu)
    if p.kernel == 1:
        bs = [1, 7, 2 * num_cu, 2 * num_cu + 1]
        if big:
            bs.append(8 * num_cu + 11)                    # some waves walk a second sample
        return bs
    gx = path(H, W, bf16, 1 << 20, num_cu).gx             # the grid of a batch that fills it
    return [1, 2, gx + 1, 2 * gx + 3]                      # gx + 1: one workgroup loops twice, the others drop a prefetched plane


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _seed(H, W, salt):
    return salt * 1000003 + H * 1009 + W


def _set(model, draw):
    """draw(kind, shape) -> tensor for kind in (w1, b1, w2, b2), per branch"""
    import torch
    with torch.no_grad():
        for br in model.branches:
            br[0].conv.weight.copy_(draw("w1", br[0].conv.weight.shape))
            br[0].conv.bias.copy_(draw("b1", br[0].conv.bias.shape))
            br[1].conv.weight.copy_(draw("w2", br[1].conv.weight.shape))
            br[1].conv.bias.copy_(draw("b2", br[1].conv.bias.shape))
    return model.eval()


@functools.lru_cache(maxsize=None)
def int_model(H, W):
    """small-integer weights: w1 in -2..2 at 60 % density, b1 in -3..3, w2 in -2..2 at 25 % density, b2 in -8..8 -- conv1 values are
    integers of magnitude <= 9 * 2 * 3 + 3 = 57, conv2 sums of magnitude <= 576 * 2 * 57 + 8 < 2^17"""
    import torch
    g = torch.Generator().manual_seed(_seed(H, W, 1))
    lim = {"w1": (2, 0.6), "b1": (3, 1.0), "w2": (2, 0.25), "b2": (8, 1.0)}

    def draw(kind, shape):
        top, density = lim[kind]
        v = torch.randint(-top, top + 1, tuple(shape), generator=g).float()
        return v * (torch.rand(tuple(shape), generator=g) < density).float()
    return _set(dnn_module().Classifier([(H, W, 1)] * 3, 3), draw)


@functools.lru_cache(maxsize=None)
def frac_model(H, W):
    """:func:`int_model` with k / 256 added to every conv1 bias (|k| <= 255): biases of up to 10 significant bits -- exact in float32
    and in the rf kernel's three bf16 slots, NOT in the LDS kernel's one.  Everything stays a multiple of 2^-8 of magnitude below
    2^16, i.e. exact in float32 in any order, so these cases are bit for bit as well -- and a bias that lost bits anywhere shows."""
    import copy
    import torch
    g = torch.Generator().manual_seed(_seed(H, W, 5))
    m = copy.deepcopy(int_model(H, W))
    with torch.no_grad():
        for br in m.branches:
            br[0].conv.bias.add_(torch.randint(-255, 256, tuple(br[0].conv.bias.shape), generator=g).float() / 256.0)
    return m


def exact_model(H, W, frac):
    return frac_model(H, W) if frac else int_model(H, W)


def _nonzero_edges(x, fill):
    for sl in ((Ellipsis, 0, slice(None)), (Ellipsis, -1, slice(None)), (Ellipsis, slice(None), 0), (Ellipsis, slice(None), -1)):
        e = x[sl]
        e[e == 0] = fill
    return x


@functools.lru_cache(maxsize=None)
def int_planes(H, W):
    """three (DISTINCT, H, W) float32 plane sets of integers in -3..3, the first and last rows and columns non-zero (a symmetric pad
    instead of TensorFlow's bottom / right one shows)"""
    import torch
    g = torch.Generator().manual_seed(_seed(H, W, 2))
    return tuple(_nonzero_edges(torch.randint(-3, 4, (DISTINCT, H, W), generator=g).float(), 1.0) for _ in range(3))


@functools.lru_cache(maxsize=None)
def real_model(H, W):
    """weights as tests/sgan_infer_common.make_model draws them: kernels N(0, sqrt(2) / sqrt(fan_in)), biases N(0, 0.2)"""
    import torch
    g = torch.Generator().manual_seed(_seed(H, W, 3))

    def draw(kind, shape):
        shape = tuple(shape)
        if kind[0] == "b":
            return torch.randn(shape, generator=g) * 0.2
        return torch.randn(shape, generator=g) * (2.0 ** 0.5 / float(np.prod(shape[1:])) ** 0.5)
    return _set(dnn_module().Classifier([(H, W, 1)] * 3, 3), draw)


@functools.lru_cache(maxsize=None)
def real_planes(H, W):
    """three (DISTINCT, H, W) float32 plane sets uniform in [-1, 1] with non-zero edges"""
    import torch
    g = torch.Generator().manual_seed(_seed(H, W, 4))
    return tuple(_nonzero_edges(torch.rand((DISTINCT, H, W), generator=g) * 2 - 1, 0.5) for _ in range(3))


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------
def round_bf16(x):
    """round-to-nearest-even of a float64 / float32 tensor to bf16's 8 significant bits, in the tensor's own dtype, straight from its
    bits (no float32 stop on the way from float64: no double rounding).  Normal numbers only -- the values here are far from both ends."""
    import torch
    if x.dtype == torch.float32:
        return x.to(torch.bfloat16).to(torch.float32)
    assert x.dtype == torch.float64
    drop = 52 - 7
    b = x.contiguous().view(torch.int64)
    b = b + ((1 << (drop - 1)) - 1) + ((b >> drop) & 1)
    b = b & ~((1 << drop) - 1)
    return b.view(torch.float64)


def bf16_bits(x):
    """the int16 bit patterns of bf16-representable values"""
    import torch
    return x.to(torch.float32).to(torch.bfloat16).view(torch.int16)


def conv1_image(model, planes, bias_bf16, dtype=None):
    """per branch the (n, 64, H/2, W/2) conv1 values BEFORE the bf16 rounding, on the kernel's operands (see :func:`twin`)"""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    bf = lambda t: t.detach().float().to(torch.bfloat16).to(dtype)
    out = []
    for x, br in zip(planes, model.branches):
        b1 = br[0].conv.bias.detach().float()
        b1 = bf(b1) if bias_bf16 else b1.to(dtype)
        out.append(F.conv2d(F.pad(bf(x)[:, None], (0, 1, 0, 1)), bf(br[0].conv.weight), b1, stride=2))
    return out


def twin(model, planes, bias_bf16, dtype=None, c1_bf16=True):
    """The two layers in ``dtype`` (float64; float32 for the summation-order yardstick) on the kernel's operands: planes, w1 and w2
    rounded to bf16; the conv1 bias as float32 (``bias_bf16`` False: k_dnn_trunk_rf, three bf16 K slots) or rounded to bf16 (True:
    k_dnn_trunk, one slot); 3x3 stride-2 convolutions with zeros on the bottom and right; conv1 rounded to bf16 (nearest even), relu;
    conv2 with the float32 b2; relu.  Returns (values before the last rounding, their bf16 bits as int16), rows in Keras' Flatten
    order (h * OW2 + w) * 96 + branch * 32 + channel.  ``c1_bf16`` False leaves the conv1 image unrounded: the float32-class kernels
    of csrc/dnn_x3.hip keep it in two or three bf16 parts."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    bf = lambda t: t.detach().float().to(torch.bfloat16).to(dtype)
    outs = []
    for c1, br in zip(conv1_image(model, planes, bias_bf16, dtype), model.branches):
        c1 = torch.relu(round_bf16(c1) if c1_bf16 else c1)
        outs.append(torch.relu(F.conv2d(F.pad(c1, (0, 1, 0, 1)), bf(br[1].conv.weight), br[1].conv.bias.detach().float().to(dtype), stride=2)))
    y = torch.cat(outs, dim=1).permute(0, 2, 3, 1).reshape(outs[0].shape[0], -1).contiguous()
    return y, bf16_bits(round_bf16(y))


@functools.lru_cache(maxsize=None)
def int_twin(H, W, frac=False, bias_bf16=False, c1_bf16=True):
    """(float64 values, bf16 bits) of the exact case of a plane shape: integer operands (the bias flag does not matter: integer biases
    are exact either way) or, ``frac``, the fractional conv1 biases of :func:`frac_model` (it does)"""
    return twin(exact_model(H, W, frac), int_planes(H, W), bias_bf16, c1_bf16=c1_bf16)


@functools.lru_cache(maxsize=None)
def real_twins(H, W, bias_bf16):
    """(float64 values, float32-twin values as float64) of the real-valued case of a plane shape"""
    import torch
    y64, _ = twin(real_model(H, W), real_planes(H, W), bias_bf16)
    y32, _ = twin(real_model(H, W), real_planes(H, W), bias_bf16, dtype=torch.float32)
    return y64, y32.double()


def to_kblock(rows, H, W):
    """(n, P * 96) rows in Keras' Flatten order -> (K / 64, n, 64) in the K-block layout: K ordered (branch, pixel, channel), P even"""
    n, P = rows.shape[0], (H // 4) * (W // 4)
    return rows.reshape(n, P, 3, 32).permute(0, 2, 1, 3).reshape(n, P * 96 // 64, 64).permute(1, 0, 2).contiguous()


def half_ulp_bf16(y):
    """half the spacing of bf16 at |y| (float64 tensor, y != 0): 2^(floor(log2 |y|) - 8)"""
    import torch
    _, e = torch.frexp(y.abs())                     # |y| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(y), e - 9)


# the real-valued cases: a plane shape for every reachable (kernel, SR, prefetch, input dtype) -- partial strips where there is a choice
REAL_SHAPES = ((24, 16), (80, 80), (124, 64), (136, 64), (196, 36), (160, 80), (60, 128), (28, 248), (36, 256))


def real_shapes():
    """[(H, W, bf16)] of the real-valued cases: REAL_SHAPES with both input dtypes where the sweep has both"""
    return [c for c in cases() if c[:2] in REAL_SHAPES]
