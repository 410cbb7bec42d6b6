"""RML_OPT_SPARSE_STORES: the projection in front of a chunk whose int8 GEMM is the sparse kernel does not store the lines of a code
row whose occupancy bit stays clear (ProjOut::skip_clear) -- the GEMM takes those from its constant line and never reads them.
A set bit's line is always fully stored, a clear bit's line may hold anything: every output must be the same bits as with whole rows,
whatever the workspaces held before."""
import numpy as np
import pytest

import sparse_rows_common as S
import sparse_stores_common as T

pytestmark = pytest.mark.gpu

M_SV = 300                      # three SV tiles, the last one partial


@pytest.fixture(scope="module")
def torch_mod(rml):
    import torch
    return torch


@pytest.fixture(scope="module")
def models(rml):
    """{grid: (arrays, GpuSVC)}, built once"""
    out = {}
    for gi, grid in enumerate(T.GRIDS):
        arrays = S.make_model(grid, M_SV, seed=500 + gi)
        out[grid] = (arrays, S.gpu_svc(rml, arrays))
    return out


def run(svc, V, torch):
    out = svc.decide_volumes(V, mode="max", scale=True, want_proba=True)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in S.OUTPUTS}


def assert_same(a, b, torch, what):
    for k in S.OUTPUTS:
        assert torch.equal(a[k], b[k]), (what, k)


def assert_oracle(out, ref, what):
    for k in ("dec_ovo", "dec_ovr", "proba"):
        err = float(np.abs(out[k].cpu().numpy() - ref[k]).max())
        print("%s: max |%s - oracle| = %.3e" % (what, k, err))
        assert err <= 1e-5, (what, k, err)              # the tolerance of test_sparse_rows_gpu.py
    for k in ("label_vote", "label_calib"):
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), (what, k)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("grid", T.GRIDS, ids=T.grid_id)
def test_holes_change_nothing(rml, rml_opt, torch_mod, models, grid, kind):
    """sparse_stores 1 against sparse_stores 0 against sparse_rows 0: all five outputs torch.equal, within 1e-5 of the float64 oracle,
    and the sparse kernel really ran."""
    torch = torch_mod
    from radar_ml_amd import _lib
    arrays, svc = models[grid]
    for B in S.BATCHES:
        Vh = S.make_frames(kind, grid, B, seed=B + 3 * len(kind))
        V = torch.from_numpy(Vh).to("cuda:0")
        ref = S.oracle(Vh, arrays)
        for chunk in (0, 512):
            what = (grid, kind, B, chunk)
            rml_opt("chunk", chunk)
            rml_opt("sparse_rows", 0)
            rml_opt("sparse_stores", 0)
            dense = run(svc, V, torch)
            rml_opt("sparse_rows", 1)
            s0 = T.store_launches(_lib)
            whole = run(svc, V, torch)
            assert T.store_launches(_lib) == s0, what           # option 0: no projection was told to skip
            rml_opt("sparse_stores", 1)
            n0 = S.sparse_launches(_lib)
            holes = run(svc, V, torch)
            assert S.sparse_launches(_lib) - n0 == (1 if chunk == 0 else -(-B // chunk)), what
            # the producer's witness: the one chunk of at least 512 rows (two frames per CU) runs the wave-per-frame kernel, which
            # writes its own words and leaves clear lines unstored; the short last chunk of chunk = 512 gets words of all ones
            assert T.store_launches(_lib) - s0 == 1, what
            assert_same(holes, whole, torch, what + ("stores 1 / stores 0",))
            assert_same(holes, dense, torch, what + ("stores 1 / sparse_rows 0",))
            assert_oracle(holes, ref, what)


@pytest.mark.parametrize("chunk", S.CHUNKS)
@pytest.mark.parametrize("grid", T.GRIDS, ids=T.grid_id)
def test_poisoned_workspaces(rml, rml_opt, torch_mod, models, grid, chunk):
    """Both workspaces hold non-background codes in every line (a batch of fully occupied frames through the same context, same B and
    chunk size) before each batch with holes runs."""
    torch = torch_mod
    from radar_ml_amd import _lib
    arrays, svc = models[grid]
    B = 1000
    junk = torch.from_numpy(S.make_frames("occupied", grid, B, seed=31)).to("cuda:0")
    rml_opt("chunk", chunk)
    rml_opt("sparse_rows", 1)
    for kind in ("blobs", "background", "mixed"):
        V = torch.from_numpy(S.make_frames(kind, grid, B, seed=32 + len(kind))).to("cuda:0")
        rml_opt("sparse_stores", 0)
        whole = run(svc, V, torch)
        rml_opt("sparse_stores", 1)
        run(svc, junk, torch)
        n0, s0 = S.sparse_launches(_lib), T.store_launches(_lib)
        assert_same(run(svc, V, torch), whole, torch, (grid, chunk, kind))
        assert S.sparse_launches(_lib) - n0 == (1 if chunk == 0 else -(-B // chunk)), (grid, chunk, kind)
        # chunks of 256 rows leave the wave-per-frame kernels (words of all ones, whole rows); 512 and 0: one chunk with holes
        assert T.store_launches(_lib) - s0 == (0 if chunk == 256 else 1), (grid, chunk, kind)


def test_poisoned_workspaces_default_rule_small_model(rml, rml_opt, torch_mod, models):
    """The default sparse_rows rule at (4, 4, 128), 1 000 rows in chunks of 512, 300 SVs: 4 x 3 and 4 x 3 tiles are fewer than the
    CUs, so BOTH chunks take split-K, which reads every line -- no chunk may get holes."""
    torch = torch_mod
    from radar_ml_amd import _lib
    grid = (4, 4, 128)
    arrays, svc = models[grid]
    B = 1000
    junk = torch.from_numpy(S.make_frames("occupied", grid, B, seed=41)).to("cuda:0")
    rml_opt("chunk", 512)
    rml_opt("sparse_rows", -1)
    for kind in ("blobs", "background", "mixed"):
        V = torch.from_numpy(S.make_frames(kind, grid, B, seed=42 + len(kind))).to("cuda:0")
        rml_opt("sparse_stores", 0)
        whole = run(svc, V, torch)
        rml_opt("sparse_stores", 1)
        run(svc, junk, torch)
        n0, s0 = S.sparse_launches(_lib), T.store_launches(_lib)
        assert_same(run(svc, V, torch), whole, torch, (kind,))
        assert S.sparse_launches(_lib) == n0 and T.store_launches(_lib) == s0, (kind,)


def test_sparse_and_dense_chunk_in_one_call(rml, rml_opt, torch_mod):
    """The per-chunk decision with a mixed plan, default sparse_rows rule: 2 000 SVs (16 SV tiles) at (4, 4, 128), 3 048 rows in
    chunks of 2 048.  The first chunk is 16 x 16 = 256 tiles -- not fewer than the CUs, so the sparse 128 x 128 kernel takes it and
    its rows get holes; the last chunk (1 000 rows, 8 x 16 tiles) takes split-K, which reads every line.  Its projection is the
    wave-per-frame kernel too (two frames per CU) and WOULD skip if told to: over poisoned workspaces the outputs equal option 0
    only if front_chunked kept that chunk's stores."""
    torch = torch_mod
    from radar_ml_amd import _lib
    grid = (4, 4, 128)
    arrays = S.make_model(grid, 2000, seed=777)
    svc = S.gpu_svc(rml, arrays)
    B, chunk = 2048 + 1000, 2048
    junk = torch.from_numpy(S.make_frames("occupied", grid, B, seed=61)).to("cuda:0")
    rml_opt("chunk", chunk)
    rml_opt("sparse_rows", -1)
    for kind in ("blobs", "background", "mixed"):
        V = torch.from_numpy(S.make_frames(kind, grid, B, seed=62 + len(kind))).to("cuda:0")
        rml_opt("sparse_stores", 0)
        run(svc, junk, torch)
        n0, s0 = S.sparse_launches(_lib), T.store_launches(_lib)
        whole = run(svc, V, torch)
        assert S.sparse_launches(_lib) - n0 == 1 and T.store_launches(_lib) == s0, (kind, "option 0")
        rml_opt("sparse_rows", 0)
        dense = run(svc, V, torch)
        rml_opt("sparse_rows", -1)
        rml_opt("sparse_stores", 1)
        run(svc, junk, torch)
        n0, s0 = S.sparse_launches(_lib), T.store_launches(_lib)
        holes = run(svc, V, torch)
        assert S.sparse_launches(_lib) - n0 == 1, kind          # first chunk sparse, last chunk split-K
        assert T.store_launches(_lib) - s0 == 1, kind           # ... and only the first chunk's projection was told to skip
        assert_same(holes, whole, torch, (kind, "stores 1 / stores 0"))
        assert_same(holes, dense, torch, (kind, "stores 1 / sparse_rows 0"))


@pytest.mark.parametrize("grid", T.GRIDS, ids=T.grid_id)
def test_clear_lines_are_not_stored(rml, rml_opt, torch_mod, grid):
    """rml_project_sparse_rows into rows prefilled with 0x55, in the pipeline's kernel configuration (600 frames in one launch)."""
    torch = torch_mod
    from radar_ml_amd import _lib
    D = S.feature_len(grid)
    KT = (D + 127) // 128
    rml_opt("project_share_cu", 1)
    for kind in ("blobs", "background", "occupied", "mixed"):
        what = (grid, kind)
        Vh = S.make_frames(kind, grid, 600, seed=5 + len(kind))
        V = torch.from_numpy(Vh).to("cuda:0")
        q_ref, occ_ref = S.project_occupancy(torch, _lib, V, grid)           # whole rows (compared with NumPy's below)
        n0 = T.store_launches(_lib)
        q, occ = T.project_sparse_rows(torch, _lib, V, grid, 1)
        assert T.store_launches(_lib) - n0 == 1, what                       # the kernel that writes its own words took the flag
        assert np.array_equal(occ, S.occupancy_rule(q_ref, D)) and np.array_equal(occ, occ_ref), what
        if kind == "background":                            # the kernel's own words, not the all-ones fill
            assert (occ[:, 0] & 1 == 0).all(), what
        bits = T.line_bits(occ, KT)
        lines, lines_ref = q.reshape(len(q), KT, 128), q_ref.reshape(len(q), KT, 128)
        assert np.array_equal(lines[bits], lines_ref[bits]), what           # every set-bit line is the whole row's
        clear = lines[~bits]
        untouched = (clear == T.POISON).all(axis=1)
        stored = (clear == T.BACKGROUND).all(axis=1)
        print("%s: %d lines, %d clear, %d of them untouched" % (what, bits.size, len(clear), int(untouched.sum())))
        assert (untouched | stored).all(), what
        if T.sparse_rows_rule(grid):
            assert untouched.all(), what
            if kind == "background":
                # only the line that holds padding -- the last xy codes and the bytes finish_wave zeroes -- was written
                assert D % 128 != 0
                assert (q[:, :128 * (KT - 1)] == T.POISON).all(), what
                assert np.array_equal(q[:, 128 * (KT - 1):], q_ref[:, 128 * (KT - 1):]), what
        # skip_clear = 0: no byte below ld is left as it was.  0x55 is itself a legal byte (code 0xD5 ^ 0x80), so "left" is judged
        # against rows computed by NumPy alone, under two different prefills: a byte the kernel did not write differs from one of them
        want = T.expected_rows(Vh, grid)
        n1 = T.store_launches(_lib)
        for fill in (T.POISON, 0xAA):
            q0, occ0 = T.project_sparse_rows(torch, _lib, V, grid, 0, fill=fill)
            assert np.array_equal(q0, want), what + (fill,)
            assert (q0[want != fill] != fill).all(), what + (fill,)             # the issue's wording, where the prefill is not the code
            assert np.array_equal(occ0, occ_ref), what + (fill,)
        assert T.store_launches(_lib) == n1, what
        assert np.array_equal(q_ref, want), what


def test_graph_capture(rml, rml_opt, torch_mod, models):
    """Captured once with sparse_stores 1 and replayed, each replay over workspaces an eager call has just filled with occupied rows."""
    torch = torch_mod
    from radar_ml_amd import _lib
    grid = T.GRIDS[0]
    arrays, svc = models[grid]
    B = 1000
    Va = torch.from_numpy(S.make_frames("blobs", grid, B, seed=51)).to("cuda:0")
    Vb = torch.from_numpy(S.make_frames("mixed", grid, B, seed=52)).to("cuda:0")
    junk = torch.from_numpy(S.make_frames("occupied", grid, B, seed=53)).to("cuda:0")
    rml_opt("chunk", 512)
    rml_opt("sparse_rows", 1)
    rml_opt("sparse_stores", 0)
    eager = {"a": run(svc, Va, torch), "b": run(svc, Vb, torch)}
    rml_opt("sparse_stores", 1)
    buf = Va.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # the warm-up on the capturing stream (torch's recipe)
        svc.decide_volumes(buf, mode="max", scale=True, want_proba=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    n0 = S.sparse_launches(_lib)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        o = svc.decide_volumes(buf, mode="max", scale=True, want_proba=True)
    assert S.sparse_launches(_lib) - n0 == 2            # both chunks' sparse GEMMs are in the captured graph
    for name, V in (("b", Vb), ("a", Va)):
        buf.copy_(V)
        run(svc, junk, torch)                               # eager, same context: both workspaces full of occupied rows
        graph.replay()
        torch.cuda.synchronize()
        assert_same(o, eager[name], torch, name)
