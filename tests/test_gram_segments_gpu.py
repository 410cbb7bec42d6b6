"""rml_gram_segments / rml_gram_compose (csrc/gram.hip): the per-segment inner products and norms of one set of float32
rows from one MFMA pass, and the kernel matrices of every union of segments composed from them, against a NumPy float64 oracle
(per segment, and of the column subset for the composed matrices); symmetry, determinism, padding and argument errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LINEAR, RBF = 0, 1
ERR_INVALID = -1
SENTINEL = -7.25


def rows(N, seg, pad=5, seed=0):
    """off-grid float32 rows in [0, 1) with ``pad`` more floats per row than the segments (NaN there: never read)"""
    D = sum(seg)
    rng = np.random.default_rng(seed + 131 * N + D)
    F = np.full((N, D + pad), np.nan, dtype=np.float32)
    F[:, :D] = rng.random((N, D), dtype=np.float32)
    return F


def parts(F, seg):
    start = np.concatenate([[0], np.cumsum(seg)])
    return [F[:, start[s]:start[s + 1]].astype(np.float64) for s in range(len(seg))]


def subset_oracle(F, seg, bits, kind, gamma):
    X = np.concatenate([p for s, p in enumerate(parts(F, seg)) if bits >> s & 1], axis=1)
    dot = X @ X.T
    if kind == LINEAR:
        return dot
    sq = (X * X).sum(1)
    return np.exp(-gamma * (sq[:, None] + sq[None, :] - 2.0 * dot))


def run_segments(F, N, seg, ld_g=None, stride_s=None):
    """rml_gram_segments on a device copy of F; returns the DEVICE buffers (G flat with sentinels, nsq)."""
    import torch
    from radar_ml_amd import _lib
    lib = _lib.load()
    ld_g = ld_g or N
    stride_s = stride_s or N * ld_g
    Fd = torch.from_numpy(F).cuda()
    G = torch.full((len(seg) * stride_s,), SENTINEL, dtype=torch.float64, device="cuda")
    nsq = torch.full((len(seg) * N + 3,), SENTINEL, dtype=torch.float64, device="cuda")
    sl = np.asarray(seg, dtype=np.int64)
    rc = lib.rml_gram_segments(_lib.context(), _lib.ptr(Fd), F.shape[1], N, len(seg), sl.ctypes.data, _lib.ptr(G), ld_g, stride_s,
                               _lib.ptr(nsq), _lib.stream_ptr())
    _lib.check(rc, "rml_gram_segments")
    torch.cuda.synchronize()
    return G, nsq


def run_compose(G, nsq, N, nseg, keys, ld_g=None, stride_s=None, ld_out=None, stride_k=None):
    """rml_gram_compose for ``keys`` = [(bits, kind, gamma)]; returns the whole output buffer (n_out, stride_k) on the host."""
    import torch
    from radar_ml_amd import _lib
    lib = _lib.load()
    ld_g = ld_g or N
    stride_s = stride_s or N * ld_g
    ld_out = ld_out or N
    stride_k = stride_k or N * ld_out
    out = torch.full((len(keys) * stride_k,), SENTINEL, dtype=torch.float64, device="cuda")
    b = np.array([k[0] for k in keys], dtype=np.int32)
    kd = np.array([k[1] for k in keys], dtype=np.int32)
    g = np.array([k[2] for k in keys], dtype=np.float64)
    rc = lib.rml_gram_compose(_lib.context(), _lib.ptr(G), ld_g, stride_s, _lib.ptr(nsq), N, nseg, len(keys), b.ctypes.data,
                              kd.ctypes.data, g.ctypes.data, _lib.ptr(out), ld_out, stride_k, _lib.stream_ptr())
    _lib.check(rc, "rml_gram_compose")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(keys), stride_k)


def mats(buf, N, ld):
    return [b[:N * ld].reshape(N, ld)[:, :N] for b in buf]


def untouched(buf, N, ld):
    for b in buf:
        full = b[:N * ld].reshape(N, ld)
        assert (full[:, N:] == SENTINEL).all() and (b[N * ld:] == SENTINEL).all()


def mask_keys(seg):
    """every non-empty mask x (LINEAR, RBF 1e-3, RBF 1/D of the mask's columns)"""
    keys = []
    for bits in range(1, 1 << len(seg)):
        D = sum(n for s, n in enumerate(seg) if bits >> s & 1)
        keys += [(bits, LINEAR, 0.0), (bits, RBF, 1e-3), (bits, RBF, 1.0 / D)]
    return keys


@pytest.mark.parametrize("N", [1, 2, 127, 129, 300])
@pytest.mark.parametrize("seg", [(1, 31, 33), (32, 64, 32), (264, 372, 46), (5,)])
def test_segments_and_compose_match_float64_oracle(rml, N, seg):
    ld_g = N + 3
    stride_s = N * ld_g + 17
    F = rows(N, seg)
    G, nsq = run_segments(F, N, seg, ld_g, stride_s)
    gbuf = G.cpu().numpy().reshape(len(seg), stride_s)
    nh = nsq.cpu().numpy()
    for Gs, ns, p in zip(mats(gbuf, N, ld_g), nh[:len(seg) * N].reshape(len(seg), N), parts(F, seg)):
        ref = p @ p.T
        assert np.abs(Gs - ref).max() <= 1e-13 * np.abs(ref).max()
        rn = (p * p).sum(1)
        assert np.abs(ns - rn).max() <= 1e-13 * np.abs(rn).max()
        assert np.array_equal(Gs, Gs.T)                     # bitwise symmetric
    untouched(gbuf, N, ld_g)                                # padding columns and the gaps between segments
    assert (nh[len(seg) * N:] == SENTINEL).all()

    keys = mask_keys(seg)
    ld_out = N + 2
    stride_k = N * ld_out + 5
    buf = run_compose(G, nsq, N, len(seg), keys, ld_g, stride_s, ld_out, stride_k)
    for K, (bits, kind, gamma) in zip(mats(buf, N, ld_out), keys):
        ref = subset_oracle(F, seg, bits, kind, gamma)
        if kind == LINEAR:
            assert np.abs(K - ref).max() <= 1e-13 * np.abs(ref).max(), (bits, kind)
        else:
            assert np.abs(K - ref).max() <= 1e-12, (bits, gamma)
        assert np.array_equal(K, K.T), (bits, kind, gamma)
    untouched(buf, N, ld_out)


def test_compose_21_outputs_in_one_call_equal_21_calls(rml):
    N, seg = 129, (264, 372, 46)
    F = rows(N, seg, pad=0)
    G, nsq = run_segments(F, N, seg)
    keys = mask_keys(seg)
    assert len(keys) == 21
    # interleave the masks so that outputs of one mask are not neighbours
    keys = keys[0::3] + keys[1::3] + keys[2::3]
    a = run_compose(G, nsq, N, 3, keys)
    for k, key in enumerate(keys):
        assert np.array_equal(run_compose(G, nsq, N, 3, [key])[0], a[k]), key
    # more outputs of one mask than a launch takes
    many = [(5, RBF, 0.001 * (i + 1)) for i in range(11)] + [(5, LINEAR, 0.0)]
    b = run_compose(G, nsq, N, 3, many)
    for k, key in enumerate(many):
        assert np.array_equal(run_compose(G, nsq, N, 3, [key])[0], b[k]), key


def test_workload_shape_repeats_and_rbf_bound(rml):
    N, seg = 1458, (3872, 5457, 682)
    D = sum(seg)
    rng = np.random.default_rng(11)
    F = rng.random((N, D), dtype=np.float32)
    gammas = [1e-5, 1e-4, 1e-3, 1e-2, 0.1]
    keys = [(7, RBF, g) for g in gammas]
    G1, n1 = run_segments(F, N, seg)
    a = run_compose(G1, n1, N, 3, keys)
    G2, n2 = run_segments(F, N, seg)
    b = run_compose(G2, n2, N, 3, keys)
    import torch
    assert torch.equal(G1, G2) and torch.equal(n1, n2) and np.array_equal(a, b)      # deterministic run to run
    assert torch.equal(G1.view(3, N, N), G1.view(3, N, N).transpose(1, 2))
    # the bound test_six_kernels_in_one_call... derives for dense rows at this D (tests/test_gram_gpu.py)
    X = F.astype(np.float64)
    dot = X @ X.T
    sq = (X * X).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * dot
    for k, g in enumerate(gammas):
        bound = max(1e-12, 8 * np.finfo(np.float64).eps * np.sqrt(D) * g * float(sq.max()))
        assert np.abs(a[k].reshape(N, N) - np.exp(-g * d2)).max() <= bound, g


def test_code_grid_rows_linear(rml):
    """rows float32(c/255), the reference's features: every product is exact in float64, so only the summation order differs"""
    rng = np.random.default_rng(3)
    N, seg = 300, (264, 372, 46)
    F = (rng.integers(0, 256, (N, sum(seg))).astype(np.float32) / np.float32(255.0))
    G, nsq = run_segments(F, N, seg)
    keys = [(bits, LINEAR, 0.0) for bits in range(1, 8)]
    for K, (bits, _, _) in zip(mats(run_compose(G, nsq, N, 3, keys), N, N), keys):
        ref = subset_oracle(F, seg, bits, LINEAR, 0.0)
        assert np.abs(K - ref).max() <= 1e-13 * np.abs(ref).max(), bits


def test_argument_errors_and_empty(rml):
    import torch
    from radar_ml_amd import _lib
    lib = _lib.load()
    ctx = _lib.context()
    N, seg = 4, np.array([3, 4, 1], dtype=np.int64)
    D = 8
    F = torch.rand((N, D), device="cuda")
    G = torch.full((3, N, N), 3.5, dtype=torch.float64, device="cuda")
    nsq = torch.full((3, N), 3.5, dtype=torch.float64, device="cuda")
    out = torch.full((2, N, N), 3.5, dtype=torch.float64, device="cuda")
    s = _lib.stream_ptr()
    i64 = lambda *v: np.array(v, dtype=np.int64)
    i32 = lambda *v: np.array(v, dtype=np.int32)

    def segments(ctx_=ctx, feat=_lib.ptr(F), ld_feat=D, n=N, nseg=3, seg_len=seg, g=_lib.ptr(G), ld_g=N, stride_s=N * N, nq=_lib.ptr(nsq)):
        return lib.rml_gram_segments(ctx_, feat, ld_feat, n, nseg, seg_len.ctypes.data if seg_len is not None else None, g, ld_g,
                                     stride_s, nq, s)

    bad = [dict(ctx_=None), dict(feat=None), dict(g=None), dict(nq=None), dict(seg_len=None), dict(nseg=0),
           dict(nseg=9, seg_len=i64(*[1] * 9), ld_feat=9), dict(seg_len=i64(3, 0, 5)), dict(seg_len=i64(3, -1, 6)),
           dict(seg_len=i64(3, 4, 2)), dict(ld_feat=D - 1), dict(ld_g=N - 1), dict(stride_s=N * N - 1), dict(n=-1)]
    for kw in bad:
        assert segments(**kw) == ERR_INVALID, kw
        assert lib.rml_last_error().decode().startswith("rml_gram_segments"), kw
    assert segments(n=0, feat=None, g=None, nq=None) == 0 and segments(n=0) == 0      # N == 0: a no-op
    torch.cuda.synchronize()
    assert bool((G == 3.5).all()) and bool((nsq == 3.5).all())                       # untouched after every refused call
    assert segments() == 0
    torch.cuda.synchronize()

    bits2, k2, g2 = i32(5, 7), i32(LINEAR, RBF), np.array([0.0, 0.5])

    def compose(ctx_=ctx, g=_lib.ptr(G), ld_g=N, stride_s=N * N, nq=_lib.ptr(nsq), n=N, nseg=3, n_out=2, bits=bits2, kinds=k2,
                gammas=g2, o=_lib.ptr(out), ld_out=N, stride_k=N * N):
        p = lambda a: a.ctypes.data if a is not None else None
        return lib.rml_gram_compose(ctx_, g, ld_g, stride_s, nq, n, nseg, n_out, p(bits), p(kinds), p(gammas), o, ld_out, stride_k, s)

    bad = [dict(ctx_=None), dict(g=None), dict(nq=None), dict(o=None), dict(bits=None), dict(kinds=None), dict(gammas=None),
           dict(nseg=0), dict(nseg=9), dict(n_out=0), dict(bits=i32(5, 0)), dict(bits=i32(8, 7)), dict(bits=i32(-1, 7)),
           dict(nseg=2, bits=i32(3, 4)), dict(kinds=i32(LINEAR, 2)), dict(kinds=i32(-1, RBF)),
           dict(gammas=np.array([0.0, np.nan])), dict(gammas=np.array([0.0, np.inf])), dict(gammas=np.array([0.0, -1.0])),
           dict(ld_g=N - 1), dict(stride_s=N * N - 1), dict(ld_out=N - 1), dict(stride_k=N * N - 1), dict(n=-1)]
    for kw in bad:
        assert compose(**kw) == ERR_INVALID, kw
        assert lib.rml_last_error().decode().startswith("rml_gram_compose"), kw
    assert compose(n=0, g=None, nq=None, o=None) == 0 and compose(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.5).all())
    # a NaN gamma is ignored for a LINEAR entry
    assert compose(n_out=1, bits=i32(7), kinds=i32(LINEAR), gammas=np.array([np.nan])) == 0
    torch.cuda.synchronize()
    X = F.cpu().numpy().astype(np.float64)
    assert np.abs(out[0].cpu().numpy() - X @ X.T).max() <= 1e-13 * (X @ X.T).max()
    assert bool((out[1] == 3.5).all())
