"""rml_gram (csrc/gram.hip): every kernel matrix of one set of float32 rows against itself from one MFMA pass over the inner
products, against a NumPy float64 oracle; symmetry, determinism, padding and argument errors."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LINEAR, RBF = 0, 1
ERR_INVALID = -1


def oracle(X, kinds, gammas):
    X64 = X.astype(np.float64)
    dot = X64 @ X64.T
    sq = (X64 * X64).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * dot
    return [dot if k == LINEAR else np.exp(-g * d2) for k, g in zip(kinds, gammas)]


def rows(N, D, ld=None, seed=0):
    """off-grid float32 rows in [0, 1) with ``ld`` floats per row (the padding holds NaN: it must never be read)"""
    rng = np.random.default_rng(seed + 131 * N + D)
    ld = ld or D
    F = np.full((N, ld), np.nan, dtype=np.float32)
    F[:, :D] = rng.random((N, D), dtype=np.float32)
    return F


def run(rml, F, N, D, kinds, gammas, ld_out=None, stride_k=None, sentinel=-7.25):
    """rml_gram on a device copy of F; returns the whole output buffer (nk, stride_k) on the host."""
    import torch
    from radar_ml_amd import _lib
    lib = _lib.load()
    ctx = _lib.context()
    ld_out = ld_out or N
    stride_k = stride_k or N * ld_out
    nk = len(kinds)
    Fd = torch.from_numpy(F).cuda()
    out = torch.full((nk * stride_k,), sentinel, dtype=torch.float64, device="cuda")
    k = np.asarray(kinds, dtype=np.int32)
    g = np.asarray(gammas, dtype=np.float64)
    rc = lib.rml_gram(ctx, _lib.ptr(Fd), F.shape[1], N, D, nk, k.ctypes.data, g.ctypes.data, _lib.ptr(out), ld_out, stride_k,
                      _lib.stream_ptr())
    _lib.check(rc, "rml_gram")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nk, stride_k)


def mats(buf, N, ld_out):
    return [b[:N * ld_out].reshape(N, ld_out)[:, :N] for b in buf]


@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 300, 1458])
@pytest.mark.parametrize("D", [1, 31, 682, 10010])
def test_gram_matches_float64_oracle(rml, N, D):
    ldf, ld_out = D + 5, N + 3
    stride_k = N * ld_out + 17
    F = rows(N, D, ldf)
    kinds, gammas = [LINEAR, RBF, RBF], [0.0, 1e-3, 1.0 / D]
    buf = run(rml, F, N, D, kinds, gammas, ld_out, stride_k)
    ref = oracle(F[:, :D], kinds, gammas)
    for K, R, kind in zip(mats(buf, N, ld_out), ref, kinds):
        if kind == LINEAR:
            assert np.abs(K - R).max() <= 1e-13 * np.abs(R).max()
        else:
            assert np.abs(K - R).max() <= 1e-12
        assert np.array_equal(K, K.T)                        # bitwise symmetric
    for b in buf:                                          # padding columns and the gap between matrices untouched
        full = b[:N * ld_out].reshape(N, ld_out)
        assert (full[:, N:] == -7.25).all() and (b[N * ld_out:] == -7.25).all()


def test_six_kernels_in_one_call_equal_six_calls_and_runs_repeat(rml):
    N, D = 1458, 10010
    F = rows(N, D)
    kinds = [LINEAR, RBF, RBF, RBF, RBF, RBF]
    gammas = [0.0, 1e-5, 1e-4, 1e-3, 1e-2, 0.1]
    a = run(rml, F, N, D, kinds, gammas)
    b = run(rml, F, N, D, kinds, gammas)
    assert np.array_equal(a, b)                             # deterministic run to run
    for k in range(6):
        one = run(rml, F, N, D, [kinds[k]], [gammas[k]])
        assert np.array_equal(one[0], a[k]), k
    # d^2 = |x_i|^2 + |x_j|^2 - 2 x_i.x_j cancels: with dense rows at D = 10 010 (|x|^2 ~ 3 400) the float64 rounding of D-term sums,
    # ~ eps sqrt(D) |x|^2, is ~1e-10 on d^2 in the kernel (MFMA order) and in the oracle (BLAS / pairwise order) alike; it reaches
    # the kernel value as gamma * that, largest on the diagonal (K = 1).  The 1e-12 bar of test_gram_matches_float64_oracle holds
    # while gamma |x|^2 stays below ~10; above it the bound scales with gamma |x|^2
    ref = oracle(F, kinds, gammas)
    sqmax = float((F.astype(np.float64) ** 2).sum(1).max())
    for k in range(1, 6):
        bound = max(1e-12, 8 * np.finfo(np.float64).eps * np.sqrt(D) * gammas[k] * sqmax)
        assert np.abs(a[k].reshape(N, N) - ref[k]).max() <= bound, k


def test_code_grid_rows_and_linear_exactness(rml):
    """rows float32(c/255), the reference's features: every product is exact in float64, so only the summation order differs"""
    rng = np.random.default_rng(3)
    N, D = 300, 682
    F = (rng.integers(0, 256, (N, D)).astype(np.float32) / np.float32(255.0))
    buf = run(rml, F, N, D, [LINEAR, RBF], [0.0, 0.01])
    ref = oracle(F, [LINEAR, RBF], [0.0, 0.01])
    K = mats(buf, N, N)
    assert np.abs(K[0] - ref[0]).max() <= 1e-13 * np.abs(ref[0]).max()
    assert np.abs(K[1] - ref[1]).max() <= 1e-12


def test_argument_errors_and_empty(rml):
    import torch
    from radar_ml_amd import _lib
    lib = _lib.load()
    ctx = _lib.context()
    N, D = 4, 8
    F = torch.rand((N, D), device="cuda")
    out = torch.full((2, N, N), 3.5, dtype=torch.float64, device="cuda")
    k2 = np.array([LINEAR, RBF], dtype=np.int32)
    g2 = np.array([0.0, 0.5])
    fp, op, s = _lib.ptr(F), _lib.ptr(out), _lib.stream_ptr()

    def call(ctx_=ctx, feat=fp, ld_feat=D, n=N, d=D, nk=2, kinds=k2, gammas=g2, o=op, ld_out=N, stride_k=N * N):
        kp = kinds.ctypes.data if kinds is not None else None
        gp = gammas.ctypes.data if gammas is not None else None
        return lib.rml_gram(ctx_, feat, ld_feat, n, d, nk, kp, gp, o, ld_out, stride_k, s)

    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(ctx_=None), dict(feat=None), dict(o=None), dict(kinds=None), dict(gammas=None),
           dict(ld_feat=D - 1), dict(ld_out=N - 1), dict(stride_k=N * N - 1), dict(nk=0), dict(nk=9),
           dict(kinds=np.array([LINEAR, 2], dtype=np.int32)), dict(kinds=np.array([-1, RBF], dtype=np.int32)),
           dict(gammas=np.array([0.0, np.nan])), dict(gammas=np.array([0.0, np.inf])), dict(gammas=np.array([0.0, -1.0])),
           dict(n=-1), dict(d=0)]
    before = out.clone()
    for kw in bad:
        assert call(**kw) == ERR_INVALID, kw
        assert lib.rml_last_error().decode().startswith("rml_gram"), kw
    # a NaN gamma is ignored for a LINEAR entry (gamma has no meaning there)
    assert call(nk=1, kinds=np.array([LINEAR], dtype=np.int32), gammas=np.array([np.nan]), stride_k=N * N) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[1], before[1])
    # N == 0: a no-op
    out.fill_(3.5)
    assert call(n=0, feat=None, o=None) == 0
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.5).all())
