"""Shared by test_dnn_slice_cpu.py and test_dnn_slice_gpu.py: the grids, targets and volumes of the target-slice preprocessing tests
(csrc/preprocess_slice.hip, rml_dnn_preprocess_slices) and their reference -- NumPy slicing of the host volume, as the reference's
predict.py:98-107 does it, through the Pillow-exact resize."""
import numpy as np

# One grid per (WZ, WY) instantiation launch_pre3s_w selects (make_plan, csrc/preprocess.hip: the Z -> width windows fit 8 or 16 taps
# once shifted to a multiple of four, the Y -> width windows 5 or 12 taps; (8, 12) runs as (16, 12)).  (grid, rescale = (width, height)):
#   5 x 7 x 16 -> 16 x 16    Z unchanged (1 tap), Y stretched (<= 5 taps)                      -> (8, 5)
#   22 x 31 x 176 -> 80 x 80 the Walabot grid: Z shrinks 2.2 x (windows of ~10 taps), Y stretched -> (16, 5)
#   6 x 31 x 32 -> 16 x 32   Z shrinks 2 x (~9 taps + shift), Y shrinks 1.9 x (~9 taps)         -> (16, 12)
GRIDS = [((5, 7, 16), (16, 16)), ((22, 31, 176), (80, 80)), ((6, 31, 32), (16, 32))]

B = 3
KINDS = ("u8", "f32_grid", "f32_off")


def targets(grid):
    """(B, 3, 3) int32: index 0 and size-1 on every axis, negative indices (the most negative one too), two equal targets in one
    frame, two targets that differ only in k."""
    X, Y, Z = grid
    a, b, c = X // 2, Y // 3, Z // 2 + 1
    return np.array([[(0, 0, 0), (X - 1, Y - 1, Z - 1), (-X, -Y, -Z)],
                     [(a, b, c), (a, b, c), (-1, -2, -3)],
                     [(a, b, 1), (a, b, Z - 2), (X - 1, 0, Z - 1)]], dtype=np.int32)


def volumes(grid, kind, seed=0):
    """(B, X, Y, Z) host volumes: uint8; float32 holding integers 0..255; float32 with ONE frame (frame 1) off that grid -- every
    voxel of it a non-integer, one above 255 (on the planes of the frame's first target, so that it is seen)."""
    X, Y, Z = grid
    rng = np.random.default_rng(1000 * X + Z + seed)
    v = rng.integers(0, 256, (B, X, Y, Z)).astype(np.uint8)
    if kind == "u8":
        return v
    v = v.astype(np.float32)
    if kind == "f32_off":
        v[1] = v[1] * np.float32(0.731) + np.float32(0.3)
        a, b, c = targets(grid)[1, 0]
        v[1, a, b, c] = np.float32(256.5)
    return v


def numpy_planes(vol, ijk):
    """The reference's slicing on the host: ``vol`` (B, X, Y, Z), ``ijk`` (B, T, 3) -> float32 (xz, yz, xy) stacks of B*T planes,
    frame-major.  NumPy's own negative-index wrap."""
    xz, yz, xy = [], [], []
    for b in range(ijk.shape[0]):
        for (i, j, k) in ijk[b]:
            yz.append(vol[b, i, :, :]); xz.append(vol[b, :, j, :]); xy.append(vol[b, :, :, k])
    return [np.stack(p).astype(np.float32) for p in (xz, yz, xy)]


def exact_planes(nc, vol, ijk, rescale, out_dtype):
    """numpy_planes through (p - 127.5) / 127.5 and the Pillow-bit-identical resize (csrc/resize.hip): CUDA (B*T, H, W) tensors in
    ``out_dtype`` ("float32": Pillow's values; "bfloat16": those rounded)."""
    import torch
    return [nc.resize_bicubic(torch.from_numpy(p).cuda(), (rescale[1], rescale[0]), out_dtype=out_dtype) for p in numpy_planes(vol, ijk)]


def bf16_ulps(a, b, floor=2e-6):
    """distance of two bf16 tensors in units of the last place (bf16 is sign-magnitude: map the bit patterns to a monotone scale);
    values that differ by less than ``floor`` in absolute terms count as equal -- next to zero a float32 rounding error of 1e-6 is
    many bf16 'ulps' of a number that small and says nothing.  (The helper of tests/test_nn_gpu.py:545-553.)"""
    import torch

    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    d = (key(a) - key(b)).abs()
    return torch.where((a.float() - b.float()).abs() <= floor, torch.zeros_like(d), d)


def check_against_exact(got, want16, want32, what):
    """Check (a): the measure and the bounds of tests/test_nn_gpu.py:581-591 -- at most one bf16 ulp from the Pillow-exact planes
    rounded to bf16, on under 1 % of the pixels, and within 2^-8 of the float32 exact planes."""
    worst, frac, dmax = 0, 0.0, 0.0
    for pl in range(3):
        assert got[pl].shape == want16[pl].shape and got[pl].dtype == want16[pl].dtype, (what, pl)
        d = bf16_ulps(got[pl], want16[pl])
        worst = max(worst, int(d.max()))
        frac = max(frac, float((d != 0).float().mean()))
        dmax = max(dmax, float((got[pl].float() - want32[pl]).abs().max()))
    print("%s: worst %d bf16 ulp, %.4f %% of the pixels differ, max |d| to the float32 exact planes %.3e" % (what, worst, 100 * frac, dmax))
    assert worst <= 1 and frac < 0.01, (what, worst, frac)
    assert dmax <= 2.0 ** -8, (what, dmax)
