"""csrc/svm.hip against float64 references over model and batch geometry (tests/svm_geometry_common.py makes the cases).

A batch takes one of eight routes (plan_chunk, launch_small, launch_split, use_big_gemm, the path argument): the matrix-vector pair
k_svm_dot_small + k_svm_epi_small, split-K + the same epilogue, the 128 x 128 tile kernel on int8 / float64 / float32 operands, the
256 x 256 ring kernel (exact and multi-digit) and the kernel-matrix variants.  The golden models reach them at four feature lengths;
here one axis at a time walks the edges around (M=129, D=129, N=129, C=3): SV counts across the 8-row, 128- and 256-row tiles, feature
lengths across the 32-float and 128-byte K-steps, the split-K threshold (KT = 8) and the five ring slots, batches across the
small-path limit and the sample tiles, every pair-count instantiation (C = 2..6) with ragged and empty class blocks.

Bars (imported from test_svm_gpu.py, none invented): exact routes within 1e-9 * max(1, max |ref|) of ref_exact -- float64 round-off
only, against a reference without input rounding -- and within 2e-6 of ref_f32rows; f64 within 1e-9, digits within 1e-6, f32 within
TOL_F32 of ref_f32rows; the linear kernel's float routes at the project's relative bar _tol.  dec_ovr and proba at the bar of dec_ovo
(on rows whose pair values are further than the bar from zero: the vote part of both jumps where a pair value changes sign); labels
equal to the reference on every row whose margin exceeds 10 x the bar, the excluded rows at most 1 % of a case and printed; and on
EVERY row label_vote is the libsvm vote of the dec_ovo returned with it and label_calib the argmax of the proba returned with it.
The 1 % cap holds wherever the bar is a round-off bar, i.e. the margin 10 x bar is at most 1e-5 (the exact routes, f64 and digits of
the RBF kernel; tests/test_svm_geometry_cpu.py checks the cases at that margin).  The f32 route (margin 0.05 on pair values of order
1 in three to fifteen pairs) and the linear kernel's float routes (a bar relative to |dec| ~ 1e2, applied to probability gaps <= 1)
exclude a tenth of the rows and more, whatever the seed: a property of the bar, printed per case, not of the kernel.
Bit-identity: exact decision values do not depend on the route -- batch size, tile kernel, chunking, float or code rows.

One "GEOM" line per (case, path, reference) with the measured error; run with -s to see them."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import oracle_np as O
import svm_geometry_common as G
from test_svm_gpu import TOL_F32, _tol

pytestmark = pytest.mark.gpu

KEYS = ("dec_ovo", "dec_ovr", "proba", "label_vote", "label_calib")
B = G.BASE


# ---- running a route -----------------------------------------------------------------------------------------------------------------------
def _svc(rml, model, **kw):
    svc = rml.GpuSVC(model["sv"], model["dual_coef"], model["intercept"], model["n_support"], model["gamma"], model["classes"],
                     kernel=model["kernel"], calib_a=model["calib_a"], calib_b=model["calib_b"], **kw)
    assert svc.exact and svc.code_scale == 255.0
    return svc


def _host(outs):
    torch.cuda.synchronize()
    return types.SimpleNamespace(**{k: v.cpu().numpy() for k, v in zip(KEYS, (outs[0], outs[1], outs[3], outs[2], outs[4]))})


def _decide(svc, X, path):
    return _host(svc._decide(svc._rows(np.ascontiguousarray(X), check_finite=False), want_proba=True, path=path))


def _code_operand(codes):
    """biased code rows as process_volumes(..., codes=True) lays them out: byte = c ^ 0x80, 128-byte K-steps, zero padding"""
    N, D = codes.shape
    q = np.zeros((N, (D + 127) // 128 * 128), dtype=np.uint8)
    q[:, :D] = codes ^ 0x80
    c = codes.astype(np.int64)
    return (torch.from_numpy(q).cuda(), torch.from_numpy(c.sum(1).astype(np.int32)).cuda(), torch.from_numpy((c * c).sum(1)).cuda())


def _decide_codes(svc, codes):
    q, isum, isq = _code_operand(codes)
    return _host(svc.decide_codes(q, isum, isq, None, want_proba=True))


def _has_digit_frame(model):
    """rml_svm_load builds the fixed-point frame of the multi-digit path for an RBF model of at most 6 class pairs whose SV values are
    not all equal (D < 32768 holds for every case here)"""
    return model["kernel"] == "rbf" and len(model["classes"]) <= 4 and model["codes"].max() > model["codes"].min()


# ---- judging it ----------------------------------------------------------------------------------------------------------------------------
def _bars(model, route, ex, fr):
    """[(reference name, reference, bar)] of a route; the first entry also judges dec_ovr, proba and the labels"""
    lin = model["kernel"] == "linear"
    if route == "exact":
        return [("ref_exact", ex, 1e-9 * max(1.0, float(np.abs(ex.dec_ovo).max()))),
                ("ref_f32rows", fr, _tol(model, fr.dec_ovo) if lin else 2e-6)]
    if route == "f64":
        return [("ref_f32rows", fr, _tol(model, fr.dec_ovo, "f64") if lin else 1e-9)]
    if route == "digits":
        return [("ref_f32rows", fr, _tol(model, fr.dec_ovo, "digits") if lin else 1e-6)]
    assert route == "f32"
    return [("ref_f32rows", fr, _tol(model, fr.dec_ovo, "f32") if lin else TOL_F32)]


def _judge(tag, route, model, got, ex, fr, rows=None):
    """every assertion of one output set; ``rows`` restricts it to a subset of the batch"""
    Cn = len(model["classes"])
    sel = slice(None) if rows is None else rows
    g = types.SimpleNamespace(**{k: getattr(got, k)[sel] for k in KEYS})
    N = len(g.dec_ovo)
    assert g.dec_ovo.shape == (N, Cn * (Cn - 1) // 2) and g.proba.shape == (N, Cn)
    assert g.dec_ovr.shape == ((N,) if Cn == 2 else (N, Cn))
    # the epilogue is consistent with itself on every row, whatever the margin
    assert np.array_equal(g.label_vote, O.svm_vote_labels(g.dec_ovo, Cn)), tag
    assert np.array_equal(g.label_calib, g.proba.argmax(axis=1)), tag
    for i, (name, ref, tol) in enumerate(_bars(model, route, ex, fr)):
        r = types.SimpleNamespace(**{k: getattr(ref, k)[sel] for k in KEYS})
        err = float(np.abs(g.dec_ovo - r.dec_ovo).max())
        pair, gap = G.margins(r)
        steady = pair > tol                               # no pair value may change sign within the bar: ovr / proba are continuous there
        e_ovr = float(np.abs(g.dec_ovr - r.dec_ovr)[steady].max()) if steady.any() else 0.0
        e_pro = float(np.abs(g.proba - r.proba)[steady].max()) if steady.any() else 0.0
        keep_vote = pair > 10 * tol
        keep_cal = keep_vote & (gap > 10 * tol)
        excluded = int(N - keep_cal.sum())
        print("GEOM %s route=%s ref=%s dec_ovo=%.3e dec_ovr=%.3e proba=%.3e bar=%.1e excluded=%d/%d"
              % (tag, route, name, err, e_ovr, e_pro, tol, excluded, N))
        assert err <= tol, (tag, route, name, err, tol)
        if i == 0:
            assert e_ovr <= tol and e_pro <= tol, (tag, route, name, e_ovr, e_pro, tol)
            assert np.array_equal(g.label_vote[keep_vote], r.label_vote[keep_vote]), (tag, route)
            assert np.array_equal(g.label_calib[keep_cal], r.label_calib[keep_cal]), (tag, route)
            if 10 * tol <= G.CAP_MARGIN:
                assert excluded <= 0.01 * N, (tag, route, excluded, N)


def _same_bits(a, b, what, n=None):
    for k in KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x if n is None else x[:n], y if n is None else y[:n]), (what, k)


def _sweep(rml, c, paths=G.PATHS, code_rows=True, tag=None):
    """every path of one case against its references; returns the outputs of the exact route"""
    tag = tag or repr(c)
    svc = _svc(rml, c.model)
    exact = None
    for path in paths:
        if path in ("auto", "i8"):
            got = _decide(svc, c.X, path)
            _judge("%s %s" % (tag, path), "exact", c.model, got, c.exact, c.f32)
            if exact is not None:
                _same_bits(got, exact, "%s: i8 against auto" % tag)
            exact = got
        elif path == "digits" and not _has_digit_frame(c.model):
            with pytest.raises(rml.RadarMLError, match="no digit frame"):           # a clean RML_ERR_STATE, not a wrong answer
                svc._decide(svc._rows(c.Xoff), path="digits")
        else:
            _judge("%s %s" % (tag, path), path, c.model, _decide(svc, c.Xoff, path), None, c.f32off)
    if code_rows and exact is not None:
        got = _decide_codes(svc, c.codes)
        _judge("%s codes" % tag, "exact", c.model, got, c.exact, c.f32)
        _same_bits(got, exact, "%s: code rows against float rows" % tag)
    return exact


# ---- the star: one axis at a time ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", G.KERNELS)
@pytest.mark.parametrize("M", G.M_AXIS)
def test_sv_count_axis(rml, M, kernel):
    """M across the 8-row groups of the matrix-vector kernel and the 128- / 256-row SV tiles; M < C leaves class blocks empty"""
    _sweep(rml, G.case(M, B["D"], B["C"], B["N"], "balanced", kernel))


@pytest.mark.parametrize("kernel", G.KERNELS)
@pytest.mark.parametrize("D", G.D_AXIS)
def test_feature_length_axis(rml, D, kernel):
    """D across the 32-float and 128-byte K-steps, both parities of the step counts (the extra stride step), KT = 7 | 8 (split-K on)"""
    _sweep(rml, G.case(B["M"], D, B["C"], B["N"], "balanced", kernel))


_whole = {}


def _whole_batch(rml, D):
    """the N_MAX-row on-grid batch of the N axis, decided once per D with the default options"""
    if D not in _whole:
        c = G.case(B["M"], D, B["C"], G.N_MAX)
        _whole[D] = _decide(_svc(rml, c.model), c.X, "auto")
    return _whole[D]


@pytest.mark.parametrize("D", G.N_AXIS_D)
@pytest.mark.parametrize("n", G.N_AXIS)
def test_batch_size_axis(rml, n, D):
    """N across the matrix-vector limit (8) and the sample tiles, at D = 129 (tile kernel) and D = 1025 (split-K); the first n rows of the
    513-row batch get the bits they have inside it"""
    exact = _sweep(rml, G.case(B["M"], D, B["C"], G.N_MAX).first(n))
    _same_bits(exact, _whole_batch(rml, D), "n=%d against the %d-row batch" % (n, G.N_MAX), n)


@pytest.mark.parametrize("Cn,pattern", G.C_AXIS)
def test_class_count_axis(rml, Cn, pattern):
    """every pair-count instantiation (PT = 1, 3, 6, 10, 15); a class block of one row; a class without support vectors"""
    _sweep(rml, G.case(B["M"], B["D"], Cn, B["N"], pattern))


# ---- corners -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,Cn,N,pattern", G.CORNERS)
def test_corners(rml, M, D, Cn, N, pattern):
    _sweep(rml, G.case(M, D, Cn, N, pattern))


@pytest.mark.parametrize("M,D,Cn,N", G.ring_cases())
def test_ring_kernel_on_both_sides_of_its_five_slots(rml, rml_opt, M, D, Cn, N):
    """k_svm_gemm_ring forced (gemm_big = 1) at KT = 1, 2, 3, 5, 5, 9 -- fewer K-steps than ring slots, as many, more -- on ragged N and M:
    against the references, and the bits of the 128 x 128 / split-K kernels (gemm_big = 0)"""
    c = G.case(M, D, Cn, N)
    rml_opt("gemm_big", 0)
    small_tiles = _sweep(rml, c, paths=("auto",), code_rows=False, tag="%r big=0" % c)
    rml_opt("gemm_big", 1)
    ring = _sweep(rml, c, paths=("auto", "i8", "digits"), tag="%r big=1" % c)
    _same_bits(ring, small_tiles, "%r: ring against the 128-row tiles" % c)


@pytest.mark.parametrize("big", [0, 1])
def test_mixed_batch_takes_each_tile_group_down_its_own_route(rml, rml_opt, big):
    """auto path, 513 rows of which 300..419 are off the code grid: the tile predicate (per 128 rows, per 256 under gemm_big = 1) sends
    rows 256..511 to the float64 kernel and leaves the rest on the exact one"""
    c = G.case(B["M"], B["D"], B["C"], G.N_MAX)
    whole = _whole_batch(rml, B["D"])                    # default options, every row on the grid
    X = c.X.copy()
    X[300:420] *= G.OFF_GRID
    rml_opt("gemm_big", big)
    got = _decide(_svc(rml, c.model), X, "auto")
    general = np.arange(256, 512)
    fr = G.ref_f32rows(c.model, X[general])
    g = types.SimpleNamespace(**{k: getattr(got, k)[general] for k in KEYS})
    _judge("%r mixed big=%d rows 256..511" % (c, big), "f64", c.model, g, None, fr)
    on = np.r_[0:256, 512]
    _judge("%r mixed big=%d exact rows" % (c, big), "exact", c.model, got, c.exact, c.f32, rows=on)
    for k in KEYS:
        assert np.array_equal(getattr(got, k)[on], getattr(whole, k)[on]), k


@pytest.mark.parametrize("N", [129, 257])
def test_chunks_of_128_rows(rml, rml_opt, N):
    """rml_opt("chunk", 128): two or three chunks, the last of ONE row (the matrix-vector kernels inside a larger call); same bits"""
    c = G.case(B["M"], B["D"], B["C"], G.N_MAX).first(N)
    whole = _whole_batch(rml, B["D"])                    # decided with the default chunking
    rml_opt("chunk", 128)
    exact = _sweep(rml, c, tag="%r chunk=128" % c)
    _same_bits(exact, whole, "chunk=128 against the default", N)


def test_tile_kernel_and_split_k_give_the_same_bits_at_kt_9(rml):
    """D = 1025 (KT = 9): up to 2048 rows split-K takes the batch, beyond it k_svm_gemm<i8>; the 513 rows five times over land on the tile
    kernel and keep their bits"""
    c = G.case(B["M"], 1025, B["C"], G.N_MAX)
    got = _decide(_svc(rml, c.model), np.tile(c.X, (5, 1)), "auto")
    whole = _whole_batch(rml, 1025)
    for rep in (0, 4):
        for k in KEYS:
            assert np.array_equal(getattr(got, k)[rep * G.N_MAX:(rep + 1) * G.N_MAX], getattr(whole, k)), (k, rep)
    _judge("%r x5" % c, "exact", c.model, got, c.exact, c.f32, rows=slice(0, G.N_MAX))


# ---- rml_svm_kernel_matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D,N", G.KMAT_SHAPES)
def test_kernel_matrix_values_and_bounds(rml, M, D, N):
    """K(X, SV) of the kmat instantiations against the references, written through the C ABI into a sentinel-filled (N + 1) x (M + 3)
    buffer with ld_k = M + 3: columns >= M and row N stay untouched"""
    from radar_ml_amd import _lib
    lib = _lib.load()
    c = G.case(M, D, 3, N)
    svc = _svc(rml, c.model)
    want_f64 = O.svm_kernel_values(c.Xoff, c.model["sv"], c.model["gamma"])
    for path, X, bars in (("auto", c.X, [(c.exact.K, 1e-9), (c.f32.K, 2e-6)]), ("i8", c.X, [(c.exact.K, 1e-9), (c.f32.K, 2e-6)]),
                          ("f64", c.Xoff, [(want_f64, 1e-9)])):
        K = svc.kernel_matrix(X, path=path).cpu().numpy()
        assert K.shape == (N, M)
        for ref, tol in bars:
            err = float(np.abs(K - ref).max())
            print("GEOM %r kmat %s: max |K - ref| = %.3e (bar %.0e)" % (c, path, err, tol))
            assert err <= tol * max(1.0, float(np.abs(ref).max())), (path, err)
        Xd = svc._rows(X)
        buf = torch.full((N + 1, M + 3), -7.25, dtype=torch.float64, device=Xd.device)
        _lib.check(lib.rml_svm_kernel_matrix(svc._ctx, svc._h, _lib.PATHS[path], _lib.ptr(Xd), Xd.stride(0), N, _lib.ptr(buf), M + 3,
                                             _lib.stream_ptr(Xd.device)), "rml_svm_kernel_matrix")
        torch.cuda.synchronize()
        full = buf.cpu().numpy()
        assert np.array_equal(full[:N, :M], K), path                    # the same values whatever the leading dimension
        assert (full[:N, M:] == -7.25).all() and (full[N] == -7.25).all(), path


@pytest.mark.parametrize("Cn", G.KMAT_F64_C)
def test_kernel_matrix_f64_for_every_pair_count(rml, Cn):
    """k_svm_gemm<PATH_F64, PT, KM> for PT = 1, 6, 10, 15 (KMAT_SHAPES runs PT = 3) at (M, D, N) = (129, 33, 129): two SV tiles and two
    sample tiles, each with a one-row tail (padded SV rows, clamped sample rows), two K-steps; same bar and sentinel check as above"""
    from radar_ml_amd import _lib
    lib = _lib.load()
    M, D, N = G.KMAT_F64_SHAPE
    c = G.case(M, D, Cn, N)
    svc = _svc(rml, c.model)
    want = O.svm_kernel_values(c.Xoff, c.model["sv"], c.model["gamma"])
    K = svc.kernel_matrix(c.Xoff, path="f64").cpu().numpy()
    assert K.shape == (N, M)
    err = float(np.abs(K - want).max())
    print("GEOM %r kmat f64: max |K - ref| = %.3e (bar 1e-09)" % (c, err))
    assert err <= 1e-9 * max(1.0, float(np.abs(want).max())), err
    Xd = svc._rows(c.Xoff)
    buf = torch.full((N + 1, M + 3), -7.25, dtype=torch.float64, device=Xd.device)
    _lib.check(lib.rml_svm_kernel_matrix(svc._ctx, svc._h, _lib.PATHS["f64"], _lib.ptr(Xd), Xd.stride(0), N, _lib.ptr(buf), M + 3,
                                         _lib.stream_ptr(Xd.device)), "rml_svm_kernel_matrix")
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    assert np.array_equal(full[:N, :M], K)
    assert (full[:N, M:] == -7.25).all() and (full[N] == -7.25).all()


# ---- the fused front door ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 128])
@pytest.mark.parametrize("planes", ["xz+yz+xy", "xy"])
def test_fused_front_door_on_a_tiny_grid(rml, rml_opt, planes, chunk):
    """decide_volumes, grid (3, 5, 7), max mode, all three planes (D = 71) and xy alone (D = 15), integer volumes as float32 and as uint8,
    M = 130, 1 .. 257 frames (single-tile front: matrix-vector and tile kernels; chunked two-stream front, with chunks of 128 frames
    too): against ref_exact on the oracle's max-projection codes, the same bits from both ingest types and from the two-step route"""
    X, Y, Z = 3, 5, 7
    mask = rml.ProjMask(True, True, True) if planes != "xy" else rml.ProjMask(False, False, True)
    D = rml.feature_len(X, Y, Z, mask)
    assert D == (71 if planes != "xy" else 15)
    model = G.make_model(5, 130, D, 3)
    svc = _svc(rml, model)
    rng = np.random.default_rng(D)
    vol = (rng.integers(0, 256, (257, X, Y, Z)) * (rng.random((257, X, Y, Z)) < 0.1)).astype(np.uint8)
    xz, yz, xy = O.project_max(vol)
    codes = np.concatenate([p.reshape(257, -1) for p, keep in zip((xz, yz, xy), mask) if keep], axis=1)
    assert codes.shape == (257, D) and codes.dtype == np.uint8
    ex, fr = G.ref_exact(model, codes), G.ref_f32rows(model, G.on_grid(codes))
    if chunk:
        rml_opt("chunk", chunk)
    for nb in (1, 8, 9, 129, 257):
        cut = lambda ref: types.SimpleNamespace(**{k: v[:nb] for k, v in vars(ref).items()})
        v32 = torch.from_numpy(vol[:nb].astype(np.float32)).cuda()
        o32 = svc.decide_volumes(v32, mode="max", proj_mask=mask, scale=True)
        o8 = svc.decide_volumes(torch.from_numpy(vol[:nb]).cuda(), mode="max", proj_mask=mask, scale=True)
        torch.cuda.synchronize()
        got = types.SimpleNamespace(**{k: o32[k].cpu().numpy() for k in KEYS})
        _judge("front %s chunk=%d B=%d" % (planes, chunk, nb), "exact", model, got, cut(ex), cut(fr))
        for k in KEYS:
            assert torch.equal(o8[k], o32[k]), (k, nb)
        _, q, isum, isq, flags = rml.process_volumes(v32, mode="max", proj_mask=mask, scale=True, codes=True)
        assert np.array_equal((q[:, :D] ^ 0x80).cpu().numpy(), codes[:nb])
        two = _host(svc.decide_codes(q, isum, isq, flags, want_proba=True))
        _same_bits(two, got, "front %s B=%d: code rows of process_volumes" % (planes, nb))


# ---- k_linear ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 33, 129, 1025])
def test_linear_classifier_geometry(rml, D):
    """GpuLinearClassifier (k_linear: a wave per row, 64 features per step) for 2..6 classes and 1, 129, 300 rows against
    oracle_np.linear_decision in float64"""
    for Cn in (2, 3, 4, 5, 6):
        rng = np.random.default_rng([D, Cn])
        rows_c = 1 if Cn == 2 else Cn
        coef, icpt = rng.uniform(-1.0, 1.0, (rows_c, D)), rng.uniform(-0.5, 0.5, rows_c)
        clf = rml.GpuLinearClassifier(coef, icpt, np.arange(Cn))
        Xall = rng.random((300, D), dtype=np.float32)
        for N in (1, 129, 300):
            X = Xall[:N]
            ref = O.linear_decision(X, coef, icpt)
            tol = 1e-9 * max(1.0, float(np.abs(ref).max()))
            dec = clf.decision_function(X)
            lab = clf.predict(X)
            if Cn == 2:
                ref = ref[:, 0]
                margin, want = np.abs(ref), (ref > 0).astype(np.int64)
            else:
                top = np.sort(ref, axis=1)
                margin, want = top[:, -1] - top[:, -2], ref.argmax(axis=1)
            assert dec.shape == ref.shape
            err = float(np.abs(dec - ref).max())
            keep = margin > 10 * tol
            print("GEOM k_linear D=%d C=%d N=%d: max |dec - ref| = %.3e (bar %.1e) excluded=%d/%d" % (D, Cn, N, err, tol, N - keep.sum(), N))
            assert err <= tol
            assert np.array_equal(lab[keep], want[keep]) and (N - keep.sum()) <= 0.01 * N
