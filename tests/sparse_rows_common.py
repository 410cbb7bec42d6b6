"""Helpers of tests/test_sparse_rows_gpu.py: small frames with controlled background, models on the code grid, the float64
oracle of the fused path and a NumPy restatement of the occupancy rule (include/radarml.h, RML_OPT_SPARSE_ROWS)."""
import ctypes

import numpy as np

# (X, Y, Z): k_project_wave with 9 K-steps (D = 1 040, the last one holds padding) and with 5 (D = 528); the k_project_lin family
GRIDS = ((4, 4, 128), (4, 4, 64), (4, 17, 176))
KINDS = ("blobs", "background", "occupied", "mixed")
MODELS = (128, 130, 300)        # SVs: one tile, a two-row tail tile, three tiles
BATCHES = (640, 1000)           # the last sample tile is partial
# rows per chunk: 256 rotates several chunks through both workspaces (chunks below two frames per CU leave the wave-per-frame
# kernels: their occupancy words are all ones); 512 and 0 (one chunk) keep the wave-per-frame kernels and their own words
CHUNKS = (256, 512, 0)


def feature_len(grid):
    X, Y, Z = grid
    return X * Z + Y * Z + X * Y


def make_frames(kind, grid, B, seed):
    """(B, X, Y, Z) float32 frames of integer codes.  blobs: a few voxels per frame, so that most 128-byte lines of a code row are
    background and some are not; background: all zero; occupied: no zero anywhere; mixed: blobs with one frame off the code grid
    (+ 0.5) in every other 128-row sample tile, so that those tiles fall to the float64 path beside sparse int8 tiles."""
    X, Y, Z = grid
    rng = np.random.default_rng(seed)
    if kind == "background":
        return np.zeros((B, X, Y, Z), dtype=np.float32)
    if kind == "occupied":
        return rng.integers(1, 256, (B, X, Y, Z)).astype(np.float32)
    V = np.zeros((B, X, Y, Z), dtype=np.float32)
    n = rng.integers(0, 4, B)                                   # 0 .. 3 returns per frame
    for t in range(3):
        on = np.nonzero(n > t)[0]
        V[on, rng.integers(0, X, len(on)), rng.integers(0, Y, len(on)), rng.integers(0, Z, len(on))] = rng.integers(1, 256, len(on))
    if kind == "mixed":
        V[133::256, 0, 0, 0] += 0.5                     # frames 133, 389, ...: tiles 1, 3, ... of the batch (chunks are whole tiles)
    return V


def make_model(grid, M, seed):
    """A 3-class RBF model whose M support vectors are code rows with mostly-background lines (and a few rows without any)."""
    D = feature_len(grid)
    rng = np.random.default_rng(seed)
    codes = np.zeros((M, D), dtype=np.uint8)
    for r in range(M):
        for k in rng.choice((D + 127) // 128, size=rng.integers(0, 4), replace=False):
            lo, hi = 128 * k, min(D, 128 * k + 128)
            codes[r, rng.integers(lo, hi, 5)] = rng.integers(1, 256, 5)
    codes[1::16] = rng.integers(1, 256, (len(codes[1::16]), D))   # fully occupied rows
    sv = (codes.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    ns = np.array([M // 3, M // 3, M - 2 * (M // 3)], dtype=np.int32)
    return dict(codes=codes, sv=sv, dual_coef=rng.uniform(-2, 2, (2, M)), intercept=np.array([0.1, -0.2, 0.3]), n_support=ns, gamma=0.5,
                classes=np.arange(3), calib_a=-np.ones(3), calib_b=np.zeros(3))


def gpu_svc(rml, model):
    return rml.GpuSVC(model["sv"], model["dual_coef"], model["intercept"], model["n_support"], model["gamma"], model["classes"],
                      calib_a=model["calib_a"], calib_b=model["calib_b"], device="cuda:0")


def oracle(V, model):
    """float64 restatement of decide_volumes(mode='max', scale=True, want_proba=True)"""
    import oracle_c as OC
    xz, yz, xy = OC.project_max(V, threads=2)
    return OC.svm(OC.features(xz, yz, xy, scale=True), model["sv"], model["dual_coef"], model["intercept"], model["n_support"],
                  model["gamma"], "rbf", model["calib_a"], model["calib_b"], threads=2)


OUTPUTS = ("dec_ovo", "dec_ovr", "proba", "label_vote", "label_calib")


def occupancy_rule(rows, D):
    """rows: (R, >= ceil(D / 128) * 128) uint8 BIASED code rows (byte = code ^ 0x80).  One bit per 128-byte line, bit k & 31 of dword
    k >> 5: 1 unless all 128 bytes are 0x80 and the line lies wholly inside D."""
    KT = (D + 127) // 128
    ow = (KT + 31) // 32
    out = np.zeros((rows.shape[0], ow), dtype=np.uint32)
    for k in range(KT):
        bg = (rows[:, 128 * k:128 * k + 128] == 0x80).all(axis=1) & (128 * (k + 1) <= D)
        out[:, k >> 5] |= (~bg).astype(np.uint32) << np.uint32(k & 31)
    return out


def sparse_launches(lib_mod):
    """sparse GEMM launches the current device's context has issued so far"""
    return int(lib_mod.load().rml_ctx_sparse_gemm_launches(lib_mod.context()))


def sv_occupancy(lib, svc, D):
    """the model's occupancy words: (Mpad, words) uint32"""
    ow = ((D + 127) // 128 + 31) // 32
    mpad = (svc.n_sv + 127) // 128 * 128
    out = np.zeros((mpad, ow), dtype=np.uint32)
    rc = lib.rml_svm_sv_occupancy(svc._ctx, svc._h, out.ctypes.data_as(ctypes.c_void_p), out.size)
    assert rc == 0, lib.rml_last_error()
    return out


def project_occupancy(torch, lib_mod, V, grid):
    """code rows and occupancy words of the frames V (a CUDA tensor) through rml_project_occupancy: (q uint8 (B, ld), occ int32 (B, words))"""
    lib = lib_mod.load()
    X, Y, Z = grid
    D = feature_len(grid)
    B = V.shape[0]
    ld = (D + 127) // 128 * 128
    ow = ((D + 127) // 128 + 31) // 32
    q = torch.full((B, ld), 0x55, dtype=torch.uint8, device=V.device)
    occ = torch.full((B, ow), 0x5A5A5A5A, dtype=torch.int32, device=V.device)
    isum = torch.empty(B, dtype=torch.int32, device=V.device)
    isq = torch.empty(B, dtype=torch.int64, device=V.device)
    flags = torch.empty(B, dtype=torch.int32, device=V.device)
    lib_mod.check(lib.rml_project_occupancy(lib_mod.context(V.device), V.data_ptr(), 0, B, X, Y, Z, 0, 255.0, 7, q.data_ptr(), ld,
                                            isum.data_ptr(), isq.data_ptr(), flags.data_ptr(), occ.data_ptr(), ow,
                                            lib_mod.stream_ptr(V.device)), "rml_project_occupancy")
    torch.cuda.synchronize()
    return q.cpu().numpy(), occ.cpu().numpy().view(np.uint32)
