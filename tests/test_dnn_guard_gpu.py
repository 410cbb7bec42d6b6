"""The margin guard's device side on the GPU: csrc/guard.hip against the stand-in the CPU tests drive the policy with
(tests/dnn_guard_common.py, written from include/radarml.h), and the routes of Classifier.rescore_exact against each other."""
import importlib

import numpy as np
import pytest
import torch

from dnn_guard_common import guard_apply, top2_gap

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(rng, N, C, ld):
    """(N, C) probabilities inside an (N, ld) buffer whose pad columns hold a sentinel"""
    buf = torch.full((N, ld), -7.0)
    buf[:, :C] = torch.softmax(torch.from_numpy(rng.normal(0, 2, (N, C)).astype(np.float32)), dim=1)
    return buf


@pytest.mark.parametrize("C", [2, 3, 16])
def test_guard_kernels_match_the_contract(rml, C):
    """rml_dnn_top2_gap and rml_dnn_guard_apply, bit for bit: table sizes around the 256-row workgroup, row strides with and without
    padding, re-scored row counts around the wave (64) and the workgroup (256) whose lanes share one atomic pair; a NaN in the old
    values, an inf in the fresh ones, exact ties in both; with and without the gap array."""
    from radar_ml_amd import _lib
    lib, ctx, st = _lib.load(), _lib.context(), _lib.stream_ptr()
    rng = np.random.default_rng(40 + C)
    thr = 0.05
    for N in (1, 255, 257, 4097):
        for ld in (C, C + 5):
            for n in (k for k in (1, 64, 65, 257) if k <= N):
                for with_gap in (True, False):
                    buf = _table(rng, N, C, ld)
                    rows = torch.from_numpy(rng.permutation(N)[:n].astype(np.int64))
                    fresh = _table(rng, n, C, C)
                    buf[rows[0], C - 1] = float("nan")                      # an old row with a NaN: a tie, and no word on the error
                    if N > 1:
                        other = int((rows[0] + 1) % N)
                        buf[other, 0] = buf[other, 1] = 0.4                 # an exact tie in the old values
                    if n > 2:
                        fresh[1, 0] = float("inf")                          # a fresh row with an inf
                        fresh[2, 0] = fresh[2, 1] = 0.45                    # an exact tie in the fresh values: close
                    d_buf, d_rows, d_fresh = buf.cuda(), rows.cuda(), fresh.cuda()
                    d_p = d_buf[:, :C]
                    d_gap = torch.empty((N,), dtype=torch.float32, device="cuda")
                    _lib.check(lib.rml_dnn_top2_gap(ctx, _lib.ptr(d_p), ld, N, C, _lib.ptr(d_gap), st), "rml_dnn_top2_gap")
                    gap = top2_gap(buf[:, :C])
                    assert torch.equal(_bits(d_gap.cpu()), _bits(gap)), (N, ld)
                    assert float(gap[rows[0]]) == 0.0
                    stats = torch.zeros((2,), dtype=torch.int32, device="cuda")
                    close = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
                    _lib.check(lib.rml_dnn_guard_apply(ctx, _lib.ptr(d_p), ld, C, _lib.ptr(d_rows), n, _lib.ptr(d_fresh), thr,
                                                       _lib.ptr(d_gap) if with_gap else None, _lib.ptr(stats), _lib.ptr(close), st), "rml_dnn_guard_apply")
                    err, still, want_close = guard_apply(buf[:, :C], rows, fresh, thr, gap if with_gap else None)
                    what = (N, ld, n, with_gap)
                    assert torch.equal(_bits(d_buf.cpu()), _bits(buf)), what                  # replaced rows, and nothing else (pad columns too)
                    sh = stats.cpu()
                    assert int(sh[0]) == int(_bits(err.reshape(1))[0]) and int(sh[1]) == still, what
                    assert torch.equal(close.cpu(), want_close), what
                    assert torch.equal(_bits(d_gap.cpu()), _bits(gap)), what                  # +inf on the re-scored rows only where asked
                    assert bool(torch.isinf(gap[rows]).all()) == with_gap


def test_cuda_ops_wrap_the_kernels(rml):
    """dnn_guard.CudaOps (what Classifier._guard hands the policy) returns what the stand-in returns"""
    G = importlib.import_module("radar_ml_amd.dnn_guard")
    rng = np.random.default_rng(50)
    N, C = 4097, 3
    buf = _table(rng, N, C, C + 1)
    buf[7, 0] = float("nan")
    d_p = buf.cuda()[:, :C]
    ops = G.CudaOps()
    d_gap = ops.gaps(d_p)
    gap = top2_gap(buf[:, :C])
    assert torch.equal(_bits(d_gap.cpu()), _bits(gap))
    cand = ops.candidates(d_gap, 0.02)
    want = G.GuardOps().candidates(gap, 0.02)
    assert torch.equal(cand.cpu(), want) and 7 in want.tolist()
    fresh = _table(rng, int(want.numel()), C, C)
    for g_dev, g_host in ((d_gap, gap), (None, None)):
        e, k, close = ops.apply(d_p, cand, fresh.cuda(), G.LABEL_GUARD_X3 * 1000, g_dev)
        we, wk, wclose = guard_apply(buf[:, :C], want, fresh, G.LABEL_GUARD_X3 * 1000, g_host)
        assert e == float(we) and k == wk and torch.equal(close.cpu(), wclose) and torch.equal(_bits(d_p.cpu()), _bits(buf[:, :C]))
    assert ops.candidates(d_gap, 0.02) is None                  # every candidate's gap is +inf now
    with pytest.raises(ValueError):
        G.CudaOps().gaps(buf[:, :C])                            # a host table


@pytest.mark.parametrize("vdtype", ["float32", "uint8"])
def test_rescore_exact_routes_agree(rml, monkeypatch, vdtype):
    """Every route of rescore_exact -- the fused sparse gather, all rows, dense blocks (the block shrunk to 64 frames: five of them), the
    unfused / host gather -- agrees with ``rescore_exact(V, "x3")[rows]``: rows sparse and dense, out of order, with repeats, and None;
    volumes on the device and on the host.  Asserted: the float32 round-off bound test_exact_features_in_one_call holds the sparse and
    the dense route to (2e-6).  Every stage makes a row's result a function of that row alone (projection, resize, x3 trunk,
    rml_dnn_dense_tail_f32), so equal bits are expected and each case prints whether it had them; the bound stays until a run of the
    routes before they were split has shown equal bits too."""
    dnn = importlib.import_module("radar_ml_amd.dnn")
    grid, rescale = (16, 24, 48), (64, 32)
    torch.manual_seed(31)
    model = dnn.Classifier([(32, 64, 1)] * 3, 3).to("cuda").eval()
    monkeypatch.setattr(dnn.Classifier, "RESCORE_BLOCK", 64)
    V, _ = rml.synth_volumes(300, *grid, seed=37)
    V = V.to(getattr(torch, vdtype))
    allp = model.rescore_exact(V, rescale, precision="x3")
    assert allp.shape == (300, 3)
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(300, generator=g)
    cases = {"sparse": torch.tensor([299, 3, 150, 7]), "sparse, repeats": torch.tensor([5, 5, 17, 5, 0]), "sparse, ascending": torch.tensor([1, 64, 65, 128]),
             "dense": perm[:200], "dense, repeats": torch.cat([perm[:180], perm[:40]]), "dense, ascending": perm[:150].sort().values,
             "dense, one block empty": torch.cat([torch.arange(0, 64), torch.arange(128, 300)])[perm[:236] % 236], "all": None}
    for host in (False, True):
        vol = V.cpu() if host else V
        for name, rows in cases.items():
            rows = rows if rows is None else rows.cuda()
            got = model.rescore_exact(vol, rescale, precision="x3", rows=rows)
            want = allp if rows is None else allp[rows]
            worst = float((got - want).abs().max())
            print("%s, %s volumes, %s: max |dp| = %.3g, equal bits: %s" % (name, "host" if host else "device", vdtype, worst, torch.equal(got, want)))
            assert got.shape == want.shape and worst < 2e-6, (name, host)
    # the unfused gather on the device: a precision the one-call route does not take
    p64 = model.rescore_exact(V, rescale, precision="float64")
    rows = cases["sparse"].cuda()
    assert float((model.rescore_exact(V, rescale, precision="float64", rows=rows) - p64[rows]).abs().max()) < 1e-12
