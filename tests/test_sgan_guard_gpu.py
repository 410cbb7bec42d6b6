"""The SGAN classifier's margin guard on the GPU: the float32-class trunk (csrc/sgan_x3.hip) and the float32 LeakyReLU tail
(csrc/dense.hip rml_dense_tail_lrelu_f32) against the float64 route on the same float32 planes and folded weights, and the guard
itself (Discriminator.forward_guarded, predict_volumes(label_guard=...)) against float64 labels on rows built to sit near a tie
(sgan_guard_common).

Measured on an MI355X over the case set below (one run; every test prints its figures):
  features, max |feat - float64| / row maximum:  x3 1.13e-5, x6 1.45e-6
  probabilities, max |p - p64|:                  x3 1.66e-5, x6 1.93e-6
"""
import copy
import functools
import importlib

import numpy as np
import pytest
import torch

import sgan_guard_common as G
from sgan_infer_common import SLOPE, make_model, make_planes

pytestmark = pytest.mark.gpu

RML_ERR_INVALID, RML_ERR_UNSUPPORTED = -1, -2
SEEDS = {(8, 8): 1, (16, 16): 2, (16, 40): 3, (40, 16): 4, (128, 128): 5}
# max |feat - float64| / row maximum over TRUNK_CASES x slopes x batches: 4 x the measured worst, rounded up to one digit.
# Measured (one run): x3 1.125e-5 ((40, 16), B = 9, slope 0.2), x6 1.446e-6 ((40, 16), B = 9, slope 0) -- the x6 figure sits on the
# float32 accumulation's own noise (sums of 1152 and 576 terms through three layers)
FEAT_X3_BOUND = 5e-5
FEAT_X6_BOUND = 6e-6
# fixed ceilings, whatever the constants say: a trunk that drops a cross term errs at bf16's 2^-9 class
FEAT_X3_CEILING = 2.0 ** -11
FEAT_X6_CEILING = 2.0 ** -18
F32_TAIL_BOUND = 2e-6           # test_nn_gpu.py test_float32_tail_is_a_function_of_the_row: rml_dnn_dense_tail_f32 against the float64 layers
TRUNK_CASES = [(H, W, B) for (H, W) in ((8, 8), (16, 16), (16, 40), (40, 16)) for B in (1, 3, 9)] + [(128, 128, 2), (128, 128, 9)]


@pytest.fixture(scope="module")
def sgan(rml):
    return importlib.import_module("radar_ml_amd.sgan")


@functools.lru_cache(maxsize=None)
def trunk_case(H, W, slope):
    """(model on the GPU with LeakyReLU(slope) everywhere, nine plane sets, float64 features, float64 probabilities), computed once"""
    model = make_model(H, W, 3, SEEDS[(H, W)], device="cuda")
    for mod in model.modules():
        if isinstance(mod, torch.nn.LeakyReLU):
            mod.negative_slope = slope
    xs = make_planes(9, H, W, SEEDS[(H, W)], device="cuda")
    assert model.folded_packs()["slope"] == slope
    return model, xs, model.features_float64(*xs), model.forward_exact(*xs, precision="float64")


def row_error(got, ref):
    """max over rows and elements of |got - ref| / the row's largest |ref|"""
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    return float(((got.double() - ref).abs() / scale).max())


@pytest.mark.parametrize("slope", [SLOPE, 0.0])
@pytest.mark.parametrize("H,W,B", TRUNK_CASES)
def test_trunk_features_against_float64(sgan, H, W, B, slope):
    """features_x3 at parts 2 and 3 against the float64 route on the same float32 planes and folded weights"""
    model, xs_all, f64_all, _ = trunk_case(H, W, slope)
    assert model.x3_supported(H, W)
    xs, f64 = [x[:B] for x in xs_all], f64_all[:B]
    f3, f6 = model.features_x3(*xs), model.features_x3(*xs, parts=3)
    assert f3.dtype == torch.float32 and f3.shape == f64.shape and f6.shape == f64.shape
    e3, e6 = row_error(f3, f64), row_error(f6, f64)
    print("x3 trunk %dx%d B=%d slope %g: max |feat - f64| / rowmax: x3 %.3e (bound %.0e), x6 %.3e (bound %.0e)" % (H, W, B, slope, e3, FEAT_X3_BOUND, e6, FEAT_X6_BOUND))
    assert e3 < FEAT_X3_CEILING and e6 < FEAT_X6_CEILING
    assert e3 <= FEAT_X3_BOUND and e6 <= FEAT_X6_BOUND
    assert torch.equal(model.features_x3(*[x.unsqueeze(1) for x in xs]), f3)          # (N, 1, H, W) planes are taken as they are
    if slope == 0.0:
        assert bool((f3 >= 0).all()) and bool((f6 >= 0).all())


def test_trunk_probabilities_against_float64(sgan):
    """forward_exact("x3" / "x6") against float64 over the case set: within a quarter of the guard's next level, i.e. LABEL_GUARD_X3 /
    LABEL_GUARD_X6 cover four times this stage's worst error"""
    worst3 = worst6 = 0.0
    for (H, W) in SEEDS:
        for slope in (SLOPE, 0.0):
            model, xs, _, p64 = trunk_case(H, W, slope)
            p3, p6 = model.forward_exact(*xs, precision="x3"), model.forward_exact(*xs, precision="x6")
            assert p3.dtype == torch.float32 and p3.shape == p64.shape
            assert torch.allclose(p3.sum(1), torch.ones(9, device="cuda"), atol=1e-5)
            e3, e6 = float((p3.double() - p64).abs().max()), float((p6.double() - p64).abs().max())
            e32 = float((model.forward_exact(*xs, precision="float32").double() - p64).abs().max())
            print("forward_exact %dx%d slope %g: |p - p64| x3 %.3e, x6 %.3e (plain float32 layers: %.3e)" % (H, W, slope, e3, e6, e32))
            worst3, worst6 = max(worst3, e3), max(worst6, e6)
            assert e3 <= sgan.LABEL_GUARD_X3 / 4 and e6 <= sgan.LABEL_GUARD_X6 / 4
    print("worst |p - p64|: x3 %.3e, x6 %.3e" % (worst3, worst6))
    assert sgan.LABEL_GUARD_X3 >= 4 * worst3
    assert sgan.LABEL_GUARD_X6 >= 4 * worst6


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("H,W", [(16, 40), (128, 128)])
def test_a_row_is_a_function_of_the_row(sgan, H, W, parts):
    """a sample's float32-class features are the same bits alone, as the first and last of a batch, in a permuted batch and on a second
    call; so are its probabilities through the float32 tail"""
    model, xs, _, _ = trunk_case(H, W, SLOPE)
    N = 9
    fv = model.features_x3(*xs, parts=parts)
    p = model._tail_float32(fv)
    assert torch.equal(fv, model.features_x3(*xs, parts=parts)) and torch.equal(p, model.forward_exact(*xs, precision="x6" if parts == 3 else "x3"))
    for i in (0, N // 2, N - 1):
        one = [x[i:i + 1] for x in xs]
        assert torch.equal(model.features_x3(*one, parts=parts)[0], fv[i])
        assert torch.equal(model._tail_float32(model.features_x3(*one, parts=parts))[0], p[i])
        others = [j for j in range(N) if j != i][:4]
        for pos in (0, 4):                          # first, last of a batch of five
            idx = torch.tensor(others[:pos] + [i] + others[pos:], device="cuda")
            assert torch.equal(model.features_x3(*[x[idx] for x in xs], parts=parts)[pos], fv[i])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(4)).cuda()
    assert torch.equal(model.features_x3(*[x[perm] for x in xs], parts=parts), fv[perm])


@pytest.mark.parametrize("parts", [2, 3])
def test_rows_on_both_sides_of_a_round_boundary(sgan, parts):
    """16 x 16 planes (one tile per sample and branch), more samples than one round of the persistent grid takes (four waves per
    workgroup, one workgroup per CU and branch): the samples on both sides of the boundary, the last and the first have the bits they
    have in a small batch"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 4 * n_cu + 5
    model = trunk_case(16, 16, SLOPE)[0]
    xs = make_planes(B, 16, 16, seed=81, device="cuda")
    fv = model.features_x3(*xs, parts=parts)
    idx = torch.tensor([4 * n_cu - 1, 4 * n_cu, 4 * n_cu + 1, B - 1, 0], device="cuda")
    sub = [x[idx] for x in xs]
    assert torch.equal(model.features_x3(*sub, parts=parts), fv[idx])
    assert row_error(fv[idx], model.features_float64(*sub)) <= (FEAT_X3_BOUND if parts == 2 else FEAT_X6_BOUND)
    assert torch.equal(model.features_x3(*xs, parts=parts), fv)


def _tail_operands(K, N, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(s, device="cuda", generator=g)
    x = r(N, K)
    fv = torch.where(x > 0, x, SLOPE * x)
    w1 = r(64, K) / K ** 0.5
    b1, w2, b2 = r(64) * 0.1, r(64, 64) / 8.0, r(64) * 0.1
    w3, b3 = r(C, 64) / 4.0, r(C) * 0.1
    return fv, w1, b1, w2, b2, w3, b3


@pytest.mark.parametrize("C", [2, 3, 16])
@pytest.mark.parametrize("N", [1, 5, 130])
@pytest.mark.parametrize("K", [192, 24576])
def test_float32_lrelu_tail_vs_float64(rml, K, N, C):
    """rml_dense_tail_lrelu_f32 against the float64 layers on the same float32 rows, within the bound rml_dnn_dense_tail_f32 is held to;
    with slope 0 it is rml_dnn_dense_tail_f32 up to the sign of a zero; a second call gives the same bits"""
    from radar_ml_amd import _lib
    lib, ctx = _lib.load(), _lib.context(torch.device("cuda", torch.cuda.current_device()))
    fv, w1, b1, w2, b2, w3, b3 = _tail_operands(K, N, C, seed=K + 7 * N + C)
    w2t = w2.t().contiguous()
    nbytes = int(lib.rml_dnn_dense_tail_f32_workspace_bytes(N, K))
    st = _lib.stream_ptr(fv.device)

    def run(slope):
        ws = torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda")
        out = torch.empty((N, C), dtype=torch.float32, device="cuda")
        if slope is None:
            rc = lib.rml_dnn_dense_tail_f32(ctx, _lib.ptr(fv), K, N, K, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2t), _lib.ptr(b2), _lib.ptr(w3),
                                            _lib.ptr(b3), C, _lib.ptr(ws), nbytes, _lib.ptr(out), st)
        else:
            rc = lib.rml_dense_tail_lrelu_f32(ctx, _lib.ptr(fv), K, N, K, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2t), _lib.ptr(b2), _lib.ptr(w3),
                                              _lib.ptr(b3), C, slope, _lib.ptr(ws), nbytes, _lib.ptr(out), st)
        _lib.check(rc, "float32 dense tail")
        torch.cuda.synchronize()
        return out

    got = run(SLOPE)
    act = lambda t: torch.where(t > 0, t, SLOPE * t)
    h = act(fv.double() @ w1.double().t() + b1.double())
    h = act(h @ w2.double().t() + b2.double())
    want = torch.softmax(h @ w3.double().t() + b3.double(), dim=-1)
    err = float((got.double() - want).abs().max())
    print("float32 LeakyReLU tail K=%d N=%d C=%d: |dp| = %.2e (bound %.0e)" % (K, N, C, err, F32_TAIL_BOUND))
    assert err <= F32_TAIL_BOUND
    assert torch.equal(got, run(SLOPE))
    relu, zero = run(None), run(0.0)
    assert torch.equal(zero, relu)                      # compares values: -0.0 == 0.0
    assert float((got - relu).abs().max()) > 1e-4       # and the two activations are two functions


def test_float32_lrelu_tail_error_codes(rml):
    from radar_ml_amd import _lib
    lib, ctx = _lib.load(), _lib.context(torch.device("cuda", torch.cuda.current_device()))
    K = 192
    fv, w1, b1, w2, b2, w3, b3 = _tail_operands(K, 4, 16, seed=3)
    w2t = w2.t().contiguous()
    ws = torch.empty((int(lib.rml_dnn_dense_tail_f32_workspace_bytes(4, K)) // 4,), device="cuda")
    out = torch.empty((4, 16), device="cuda")
    args = lambda n, k, ld, nc, nbytes: (ctx, _lib.ptr(fv), ld, n, k, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2t), _lib.ptr(b2), _lib.ptr(w3),
                                         _lib.ptr(b3), nc, SLOPE, _lib.ptr(ws), nbytes, _lib.ptr(out), None)
    assert lib.rml_dense_tail_lrelu_f32(*args(4, K - 2, K, 3, ws.numel() * 4)) == RML_ERR_UNSUPPORTED       # K % 4
    assert lib.rml_dense_tail_lrelu_f32(*args(4, K, K, 17, ws.numel() * 4)) == RML_ERR_UNSUPPORTED          # C > 16
    assert lib.rml_dense_tail_lrelu_f32(*args(4, K, K, 3, 16)) == RML_ERR_INVALID and b"workspace" in lib.rml_last_error()
    assert lib.rml_dense_tail_lrelu_f32(*args(0, K, K, 3, 0)) == 0                                          # N = 0


def test_unsupported_planes(sgan):
    """12 x 16 planes: rml_sgan_trunk_x3 returns RML_ERR_UNSUPPORTED with nothing launched, features_x3 raises, forward_exact("x3") falls
    to the float32 layers; a short workspace is RML_ERR_INVALID, B = 0 a no-op, parts other than 2 and 3 RML_ERR_INVALID"""
    from radar_ml_amd import _lib
    model = make_model(12, 16, 3, seed=41, device="cuda")
    xs = make_planes(2, 12, 16, seed=42, device="cuda")
    assert not model.x3_supported(12, 16)
    with pytest.raises(ValueError, match="12x16"):
        model.features_x3(*xs)
    assert torch.allclose(model.forward_exact(*xs, precision="x3"), model.forward_exact(*xs, precision="float32"), atol=1e-6)
    lib = _lib.load()
    good = make_model(16, 16, 3, seed=43, device="cuda")
    pk = good.folded_packs()
    feat = torch.full((2, 4 * 96), 7.0, dtype=torch.float32, device="cuda")
    nbytes = int(lib.rml_sgan_trunk_x3_workspace_bytes(2, 16, 16))
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    x16 = make_planes(2, 16, 16, seed=44, device="cuda")

    def call(planes, B, H, W, parts, wbytes):
        rc = lib.rml_sgan_trunk_x3(_lib.context(feat.device), _lib.ptr(planes[0]), _lib.ptr(planes[1]), _lib.ptr(planes[2]), B, H, W,
                                   _lib.ptr(pk["w1"]), _lib.ptr(pk["b1"]), _lib.ptr(pk["w2f"]), _lib.ptr(pk["b2"]), _lib.ptr(pk["w3f"]),
                                   _lib.ptr(pk["b3"]), SLOPE, parts, _lib.ptr(feat), _lib.ptr(ws), wbytes, _lib.stream_ptr(feat.device))
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((feat == 7.0).all()) and int(ws.count_nonzero()) == 0
    assert call(xs, 2, 12, 16, 2, nbytes) == RML_ERR_UNSUPPORTED and b"12x16" in lib.rml_last_error() and untouched()
    assert call(x16, 2, 16, 16, 2, nbytes - 16) == RML_ERR_INVALID and b"workspace" in lib.rml_last_error() and untouched()
    assert call(x16, 2, 16, 16, 4, nbytes) == RML_ERR_INVALID and untouched()
    assert call(x16, 0, 16, 16, 2, 0) == 0 and untouched()
    assert call(x16, 2, 16, 16, 2, nbytes) == 0 and torch.equal(feat, good.features_x3(*x16))
    assert good.features_x3(*[x[:0] for x in x16]).shape == (0, 4 * 96)


@pytest.mark.parametrize("spec", [G.SMALL, G.LARGE], ids=["16x16", "128x128"])
def test_guard_gives_float64_labels_on_the_fixture(sgan, spec):
    """forward_guarded on the near-tie fixture: argmax is the float64 label on EVERY row; the guard covered its gap, re-scored at
    least the rows under LABEL_GUARD and sent at least one to float64; guard off is forward_fused bit for bit"""
    cpu_model, planes, p64, gap64, _ = G.fixture(*spec)
    G.check_fixture((cpu_model, planes, p64, gap64, _))
    model = copy.deepcopy(cpu_model).to("cuda").eval()
    xs = [x.cuda() for x in planes]
    want = p64.argmax(dim=1).cuda()
    fused = model.forward_fused(*xs)
    wrong = int((fused.argmax(dim=1) != want).sum())
    print("fixture %dx%d: forward_fused alone differs from the float64 label on %d of %d rows" % (spec[0], spec[1], wrong, len(want)))
    assert torch.equal(model.forward_guarded(*xs, label_guard=None), fused) and torch.equal(model.forward_guarded(*xs, label_guard=0), fused)
    assert model.last_guard["rescored"] == 0 and model.last_guard["rounds"] == 0
    got = model.forward_guarded(*xs)
    rep = dict(model.last_guard)
    print("fixture %dx%d: last_guard = %s" % (spec[0], spec[1], rep))
    assert got.dtype == torch.float32 and got.shape == fused.shape
    assert torch.equal(got.argmax(dim=1), want), "rows %s" % (got.argmax(dim=1) != want).nonzero().flatten().tolist()
    assert rep["covered"] is True
    assert rep["rescored"] >= int((gap64 < sgan.LABEL_GUARD).sum())
    assert rep["rescored_float64"] >= 1


def test_the_fixture_bites(sgan):
    """without the guard the bf16 chain takes the other label than float64 on at least one row of the fixture (its two plane sizes
    together): the rows are close enough to a tie to show a guard that does nothing"""
    wrong = {}
    for spec in (G.SMALL, G.LARGE):
        cpu_model, planes, p64, _, _ = G.fixture(*spec)
        model = copy.deepcopy(cpu_model).to("cuda").eval()
        wrong["%dx%d" % spec[:2]] = int((model.forward_fused(*[x.cuda() for x in planes]).argmax(dim=1).cpu() != p64.argmax(dim=1)).sum())
    print("rows whose label forward_fused alone gets wrong: %s" % wrong)
    assert sum(wrong.values()) >= 1


def _tie_the_median_row(model, score64):
    """shift fc3.bias[0] of a 2-class model so that the median row's float64 logits tie to float32 rounding; returns the new float64
    probabilities of every row"""
    p = score64()
    d = torch.log(p[:, 0]) - torch.log(p[:, 1])
    m = int(torch.argsort(d)[len(d) // 2])
    with torch.no_grad():
        model.fc3.bias[0] -= d[m].float()
    return score64()


@pytest.mark.parametrize("mode", ["max", "slice"])
def test_predict_volumes_guarded(rml, sgan, mode):
    """Walabot grid -> 128 x 128, 96 synthetic frames, a 2-class model whose median row ties: with label_guard the labels are the
    float64 labels on every row (mode "slice": 192 rows, row r re-scored from frame r // 2 at ijk[r]); None is the parent's call bit
    for bit; float32 and uint8 volumes; return_numpy is kept"""
    grid, T = (22, 31, 176), 2
    V, _ = rml.synth_volumes(96, *grid, seed=91)
    model = make_model(128, 128, 2, seed=92, device="cuda")
    kw, ijk = {}, None
    if mode == "slice":
        g = torch.Generator().manual_seed(93)
        ijk = torch.stack([torch.randint(0, s, (96, T), generator=g) for s in grid], dim=-1).to(torch.int32).cuda()
        kw = {"mode": "slice", "ijk": ijk}
    rows = 96 * (T if mode == "slice" else 1)
    p64 = _tie_the_median_row(model, lambda: model.rescore_exact(V, sgan.RESCALE, mode, "float64", ijk=ijk))
    assert p64.shape == (rows, 2) and p64.dtype == torch.float64
    gap64 = (p64[:, 0] - p64[:, 1]).abs()
    print("predict_volumes %s: float64 gaps: smallest %.3e, %d of %d rows under LABEL_GUARD" % (mode, float(gap64.min()), int((gap64 < sgan.LABEL_GUARD).sum()), rows))
    assert int((gap64 < 1e-5).sum()) >= 1 and float(gap64.min()) > 0.0
    want = p64.argmax(dim=1)
    plain = model.predict_volumes(V, return_numpy=False, **kw)
    if mode == "slice":
        positional = model.predict_volumes(V, sgan.RESCALE, "slice", ijk, 8192, False, False)
    else:
        positional = model.predict_volumes(V, sgan.RESCALE, "max", None, 8192, False, False)
    assert torch.equal(model.predict_volumes(V, return_numpy=False, label_guard=None, **kw), plain) and torch.equal(positional, plain)
    assert torch.equal(model.predict_volumes(V, return_numpy=False, label_guard=0, batch_size=40, **kw), plain)
    for vol in (V, V.to(torch.uint8)):
        got = model.predict_volumes(vol, return_numpy=False, label_guard=sgan.LABEL_GUARD, **kw)
        rep = dict(model.last_guard)
        print("predict_volumes %s, %s volumes: last_guard = %s" % (mode, vol.dtype, rep))
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (rows, 2)
        assert torch.equal(got.argmax(dim=1), want), "rows %s" % (got.argmax(dim=1) != want).nonzero().flatten().tolist()
        assert rep["covered"] is True and rep["rows"] == rows and rep["rescored"] >= 1 and rep["rescored_float64"] >= 1
    as_numpy = model.predict_volumes(V.cpu().numpy(), label_guard=sgan.LABEL_GUARD, **kw)
    assert isinstance(as_numpy, np.ndarray) and as_numpy.dtype == np.float32 and np.array_equal(as_numpy.argmax(axis=1), want.cpu().numpy())
    if mode == "slice":
        # row r is frame r // T at ijk[r]: a sparse row list through rescore_exact against all rows
        pick = torch.tensor([191, 0, 77, 76, 3], device="cuda")
        assert float((model.rescore_exact(V, sgan.RESCALE, "slice", "float64", rows=pick, ijk=ijk) - p64[pick]).abs().max()) < 1e-12
        got, used = model.predict_volumes(V, return_numpy=False, return_ijk=True, label_guard=sgan.LABEL_GUARD, **kw)
        assert torch.equal(used, ijk.reshape(96, T, 3)) and torch.equal(got.argmax(dim=1), want)


def test_rescore_exact_routes_agree(rml, sgan, monkeypatch):
    """Every route of rescore_exact -- all rows, a sparse gather, dense blocks (the block shrunk to 64 frames) -- agrees with
    ``rescore_exact(V, "x3")[rows]`` to float32 round-off (the bound tests/test_dnn_guard_gpu.py holds the CNN's routes to): rows sparse
    with repeats and out of order, dense, and None; volumes on the device and on the host"""
    grid, rescale = (16, 24, 48), (64, 32)
    model = make_model(32, 64, 3, seed=95, device="cuda")
    monkeypatch.setattr(sgan.Discriminator, "RESCORE_BLOCK", 64)
    V, _ = rml.synth_volumes(300, *grid, seed=37)
    allp = model.rescore_exact(V, rescale, precision="x3")
    assert allp.shape == (300, 3) and allp.dtype == torch.float32
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(5))
    cases = {"sparse": torch.tensor([299, 3, 150, 7]), "sparse, repeats": torch.tensor([5, 5, 17, 5, 0]), "dense": perm[:200],
             "dense, repeats": torch.cat([perm[:180], perm[:40]]), "all": None}
    for host in (False, True):
        vol = V.cpu() if host else V
        for name, rows in cases.items():
            rows = rows if rows is None else rows.cuda()
            got = model.rescore_exact(vol, rescale, precision="x3", rows=rows)
            want = allp if rows is None else allp[rows]
            worst = float((got - want).abs().max())
            print("%s, %s volumes: max |dp| = %.3g, equal bits: %s" % (name, "host" if host else "device", worst, torch.equal(got, want)))
            assert got.shape == want.shape and worst < 2e-6, (name, host)
    p64 = model.rescore_exact(V, rescale, precision="float64")
    rows = cases["sparse"].cuda()
    assert float((model.rescore_exact(V, rescale, precision="float64", rows=rows) - p64[rows]).abs().max()) < 1e-12
    print("x3 against float64 on these rows: max |dp| = %.3e" % float((allp.double() - p64).abs().max()))
