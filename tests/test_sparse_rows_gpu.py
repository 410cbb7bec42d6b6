"""RML_OPT_SPARSE_ROWS: the 128 x 128 int8 GEMM of the fused pipeline stages all-background operand lines from one constant line,
by the occupancy words the projection's code stage and rml_svm_load write (csrc/mfma_tile.h SparseStager).  The operands that reach
the matrix cores are the same bytes, so every output must be the same bits as with dense staging."""
import numpy as np
import pytest

import sparse_rows_common as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod(rml):
    import torch
    return torch


@pytest.fixture(scope="module")
def models(rml):
    """{(grid, M): (arrays, GpuSVC)}, built once"""
    out = {}
    for gi, grid in enumerate(S.GRIDS):
        for M in S.MODELS:
            arrays = S.make_model(grid, M, seed=100 * gi + M)
            out[(grid, M)] = (arrays, S.gpu_svc(rml, arrays))
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
        assert err <= 1e-5, (what, k, err)
    for k in ("label_vote", "label_calib"):
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), (what, k)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("grid", S.GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_sparse_equals_dense(rml, rml_opt, torch_mod, models, grid, kind):
    """Option 1 against option 0: all five outputs torch.equal, and within 1e-5 of the float64 oracle."""
    torch = torch_mod
    from radar_ml_amd import _lib
    for B in S.BATCHES:
        Vh = S.make_frames(kind, grid, B, seed=B + len(kind))
        V = torch.from_numpy(Vh).to("cuda:0")
        for M in S.MODELS:
            arrays, svc = models[(grid, M)]
            ref = S.oracle(Vh, arrays)
            for chunk in S.CHUNKS:
                what = (grid, kind, B, M, chunk)
                rml_opt("chunk", chunk)
                rml_opt("sparse_rows", 0)
                before = S.sparse_launches(_lib)
                dense = run(svc, V, torch)
                n0 = S.sparse_launches(_lib)
                assert n0 == before, what                   # option 0 never launches the sparse kernel
                rml_opt("sparse_rows", 1)
                sparse = run(svc, V, torch)
                # forced: every chunk's exact GEMM is the sparse instantiation (one launch per chunk)
                assert S.sparse_launches(_lib) - n0 == (1 if chunk == 0 else -(-B // chunk)), what
                assert_same(sparse, dense, torch, what)
                rml_opt("sparse_rows", -1)
                assert_same(run(svc, V, torch), dense, torch, what + ("default",))
                assert_oracle(sparse, ref, what)


@pytest.mark.parametrize("chunk", S.CHUNKS)
@pytest.mark.parametrize("grid", S.GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_stale_workspace(rml, rml_opt, torch_mod, models, grid, chunk):
    """Both workspaces hold junk in every line (a batch of fully occupied frames) before the sparse batch runs."""
    torch = torch_mod
    arrays, svc = models[(grid, 300)]
    B = 1000
    V = torch.from_numpy(S.make_frames("blobs", grid, B, seed=7)).to("cuda:0")
    junk = torch.from_numpy(S.make_frames("occupied", grid, B, seed=8)).to("cuda:0")
    rml_opt("chunk", chunk)
    rml_opt("sparse_rows", 0)
    dense = run(svc, V, torch)
    rml_opt("sparse_rows", 1)
    from radar_ml_amd import _lib
    n0 = S.sparse_launches(_lib)
    run(svc, junk, torch)
    assert_same(run(svc, V, torch), dense, torch, (grid, chunk))
    assert S.sparse_launches(_lib) - n0 == 2 * (1 if chunk == 0 else -(-B // chunk)), (grid, chunk)
    zero = torch.zeros_like(V)
    rml_opt("sparse_rows", 0)
    dense0 = run(svc, zero, torch)
    rml_opt("sparse_rows", 1)
    run(svc, junk, torch)
    assert_same(run(svc, zero, torch), dense0, torch, (grid, chunk, "background"))


@pytest.mark.parametrize("grid", S.GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_occupancy_words(rml, rml_opt, torch_mod, models, grid):
    """The words read back equal the NumPy restatement of the rule: sample rows (from the projection's code stage) and SV rows."""
    torch = torch_mod
    from radar_ml_amd import _lib
    lib = _lib.load()
    D = S.feature_len(grid)
    KT = (D + 127) // 128
    # SV rows: M real rows by the rule, rows M .. Mpad (0x00) occupied in every line
    for M in S.MODELS:
        arrays, svc = models[(grid, M)]
        got = S.sv_occupancy(lib, svc, D)
        mpad = (M + 127) // 128 * 128
        assert got.shape == (mpad, (KT + 31) // 32)
        rows = np.zeros((mpad, KT * 128), dtype=np.uint8)
        rows[:M, :D] = arrays["codes"] ^ 0x80
        want = S.occupancy_rule(rows, D)
        assert np.array_equal(got, want), (grid, M)
        full = S.occupancy_rule(np.zeros((1, KT * 128), dtype=np.uint8), D)[0]
        assert (got[M:] == full).all() and (got[:M] != full).any()
    # sample rows: the pipeline's kernel configuration (one persistent workgroup per CU, the code stage), 600 frames in one launch
    rml_opt("project_share_cu", 1)
    for kind in ("blobs", "background", "occupied"):
        Vh = S.make_frames(kind, grid, 600, seed=3)
        q, occ = S.project_occupancy(torch, _lib, torch.from_numpy(Vh).to("cuda:0"), grid)
        import oracle_c as OC
        xz, yz, xy = OC.project_max(Vh, threads=2)
        codes = np.concatenate([p.reshape(len(Vh), -1) for p in (xz, yz, xy)], axis=1).astype(np.uint8)
        assert np.array_equal(q[:, :D], codes ^ 0x80) and (q[:, D:] == 0).all(), (grid, kind)
        want = S.occupancy_rule(q, D)
        assert np.array_equal(occ, want), (grid, kind)
        if kind == "background":                        # really the kernel's own words, not the all-ones fill of a kernel without a stage
            assert (occ[:, 0] & 1 == 0).all()
            assert ((occ[:, (KT - 1) >> 5] >> ((KT - 1) & 31)) & 1 == (1 if D % 128 else 0)).all()
    # a launch that leaves the wave-per-frame kernels (fewer than two frames per CU) gets words of all ones
    Vh = S.make_frames("blobs", grid, 64, seed=4)
    q, occ = S.project_occupancy(torch, _lib, torch.from_numpy(Vh).to("cuda:0"), grid)
    assert (occ == 0xFFFFFFFF).all()


def test_graph_capture(rml, rml_opt, torch_mod, models):
    """A captured-and-replayed call with option 1 returns the same bits twice."""
    torch = torch_mod
    grid = S.GRIDS[0]
    arrays, svc = models[(grid, 300)]
    B = 1000
    Va = torch.from_numpy(S.make_frames("blobs", grid, B, seed=21)).to("cuda:0")
    Vb = torch.from_numpy(S.make_frames("mixed", grid, B, seed=22)).to("cuda:0")
    rml_opt("chunk", 512)
    rml_opt("sparse_rows", 0)
    eager = {"a": run(svc, Va, torch), "b": run(svc, Vb, torch)}
    rml_opt("sparse_rows", 1)
    buf = Va.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # the warm-up on the capturing stream (torch's recipe)
        svc.decide_volumes(buf, mode="max", scale=True, want_proba=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    from radar_ml_amd import _lib
    n0 = S.sparse_launches(_lib)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        o = svc.decide_volumes(buf, mode="max", scale=True, want_proba=True)
    assert S.sparse_launches(_lib) - n0 == 2            # both chunks' sparse GEMMs are in the captured graph
    for name, V in (("b", Vb), ("a", Va), ("a", Va), ("b", Vb)):
        buf.copy_(V)
        graph.replay()
        torch.cuda.synchronize()
        assert_same(o, eager[name], torch, name)
