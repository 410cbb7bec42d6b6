"""Helpers of tests/test_sparse_stores_gpu.py (RML_OPT_SPARSE_STORES: the projection in front of a sparse chunk leaves the code-row
lines whose occupancy bit is clear unstored).  Frames, models, the oracle and the occupancy rule are sparse_rows_common's."""
import numpy as np

import sparse_rows_common as S

# (X, Y, Z), all on k_project_wave but the last.  (4, 4, 128): D = 1 040, the 16 xy bytes share the line that holds the padding -- it
# must be stored even when they are all background; (4, 4, 64): two z-rows per line (four real rows per load instruction);
# (4, 4, 256): half a z-row per line; (4, 17, 176): k_project_lin, only xz starts on a line and yz / xy straddle the lines.
GRIDS = ((4, 4, 128), (4, 4, 64), (4, 4, 256), (4, 17, 176))
POISON = 0x55                   # what the rows hold before the projection (as sparse_rows_common.project_occupancy prefills them)
BACKGROUND = 0x80


def grid_id(g):
    return "x".join(map(str, g))


def sparse_rows_rule(grid):
    """rml_sparse_rows (csrc/rml_internal.h): z-rows fill whole lines and every plane starts on a line"""
    X, Y, Z = grid
    return (Z % 128 == 0 or 128 % Z == 0) and (X * Z) % 128 == 0 and (Y * Z) % 128 == 0


def store_launches(lib_mod):
    """projection launches the current device's context has issued with skip_clear on a kernel that honours it"""
    return int(lib_mod.load().rml_ctx_sparse_store_launches(lib_mod.context()))


def expected_rows(Vh, grid):
    """(B, ld) uint8: the whole biased code rows of the frames, from NumPy alone -- max over each axis, a value that is not an integer
    in 0 .. 255 counts as code 0 (Emitter::code), byte = code ^ 0x80, the padding columns [D, ld) are 0x00"""
    D = S.feature_len(grid)
    ld = (D + 127) // 128 * 128
    planes = [Vh.max(axis=2), Vh.max(axis=1), Vh.max(axis=3)]          # xz, yz, xy
    p = np.concatenate([a.reshape(len(Vh), -1) for a in planes], axis=1).astype(np.float64)
    good = (p == np.floor(p)) & (p >= 0) & (p <= 255)
    rows = np.zeros((len(Vh), ld), dtype=np.uint8)
    rows[:, :D] = np.where(good, p, 0).astype(np.uint8) ^ 0x80
    return rows


def project_sparse_rows(torch, lib_mod, V, grid, skip_clear, fill=POISON):
    """rml_project_sparse_rows into rows prefilled with `fill`: (q uint8 (B, ld), occ uint32 (B, words))"""
    lib = lib_mod.load()
    X, Y, Z = grid
    D = S.feature_len(grid)
    B = V.shape[0]
    ld = (D + 127) // 128 * 128
    ow = ((D + 127) // 128 + 31) // 32
    q = torch.full((B, ld), fill, dtype=torch.uint8, device=V.device)
    occ = torch.full((B, ow), 0x5A5A5A5A, dtype=torch.int32, device=V.device)
    isum = torch.empty(B, dtype=torch.int32, device=V.device)
    isq = torch.empty(B, dtype=torch.int64, device=V.device)
    flags = torch.empty(B, dtype=torch.int32, device=V.device)
    lib_mod.check(lib.rml_project_sparse_rows(lib_mod.context(V.device), V.data_ptr(), 0, B, X, Y, Z, 0, 255.0, 7, q.data_ptr(), ld,
                                              isum.data_ptr(), isq.data_ptr(), flags.data_ptr(), occ.data_ptr(), ow, int(skip_clear),
                                              lib_mod.stream_ptr(V.device)), "rml_project_sparse_rows")
    torch.cuda.synchronize()
    return q.cpu().numpy(), occ.cpu().numpy().view(np.uint32)


def line_bits(occ, KT):
    """(B, KT) bool: the occupancy bit of every line"""
    k = np.arange(KT)
    return ((occ[:, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)
