"""Volumes from a foreign radar arena on the fused path: ``proj_zoom`` on process_volumes / decide_volumes (rml_project_zoom,
rml_project_zoom_svm, k_zoom_rows) against the path that existed (process_volumes at the source grid -> planes -> process_samples ->
_decide), against the reference's own library calls (SciPy's zoom on NumPy projections), against float64 and against scikit-learn.

Bars: rows 2e-7 scaled / 5e-5 unscaled (test_process_samples_nonunit_zoom_matches_reference); decisions 1e-9 on the float64 route and
1e-6 on the multi-digit route, dec_ovr and proba at the bar of dec_ovo (tests/test_svm_geometry_gpu.py)."""
import numpy as np
import pytest

import foreign_arena_common as F

pytestmark = pytest.mark.gpu

ROW_BAR = {True: 2e-7, False: 5e-5}
BAR_F64, BAR_DIGITS = 1e-9, 1e-6


def _zoom(rml, name):
    return rml.ProjZoom(*F.zoom_of(name))


def _mask(rml, bits):
    return rml.ProjMask(*F.MASKS[bits])


def _planes(rows, grid, mask):
    """source-grid feature rows (host, unscaled) -> the list of (xz, yz, xy) tuples process_samples takes (None where masked out)"""
    X, Y, Z = grid
    shapes = ((X, Z), (Y, Z), (X, Y))
    out = []
    for r in rows:
        t, off = [], 0
        for keep, (h, w) in zip(F.MASKS[mask], shapes):
            t.append(r[off:off + h * w].reshape(h, w) if keep else None)
            off += h * w if keep else 0
        out.append(tuple(t))
    return out


def _inputs(rml, name, kind, mode, B):
    """(volumes on the device, process_volumes keywords, the reference's (mode, ijk))"""
    import torch
    v = F.volumes(name, B, kind)
    vd = torch.from_numpy(np.array(v)).cuda()
    if mode == "max":
        return vd, dict(mode="max"), ("max", None)
    if mode == "slice_ijk":
        ijk = F.indices(name, B)
        return vd, dict(mode="slice", ijk=ijk), ("slice", ijk)
    if mode == "slice_t2":
        ijk = F.indices(name, B, targets=2)
        return vd, dict(mode="slice", ijk=ijk), ("slice", ijk)
    return vd, dict(mode="slice"), ("slice", F.derived_indices(v))


# (grid, volume kind, mode, mask, scale, B, context options)
ROW_CASES = [
    ("up", "int", "max", 7, True, 130, {}),                     # the row after a tile boundary
    ("up", "frac", "max", 4, False, 130, {}),
    ("up", "u8", "max", 3, True, 130, {}),
    ("up", "int", "max", 7, True, 1, {}),
    ("up", "int", "max", 7, True, 300, {"chunk": 128}),         # three chunks, the last one partial
    ("up", "u8", "slice_derived", 7, False, 300, {"chunk": 128}),
    ("up", "frac", "slice_t2", 7, False, 5, {}),
    ("up", "u8", "slice_derived", 4, True, 130, {}),
    ("up", "frac", "max", 7, True, 9, {"zoom_rows": 2}),        # one workgroup per row: one plane after the other in one LDS image
    ("up", "u8", "slice_ijk", 7, True, 9, {"zoom_rows": 1}),    # ... the images of its planes together
    ("down", "int", "slice_ijk", 7, True, 37, {}),
    ("down", "u8", "slice_ijk", 7, False, 37, {}),
    ("down", "frac", "max", 3, True, 37, {}),
    ("odd", "frac", "max", 7, True, 9, {}),
    ("odd", "u8", "slice_t2", 3, True, 9, {}),
    ("odd", "int", "slice_derived", 7, True, 9, {}),
    ("odd", "u8", "max", 4, False, 9, {}),
    ("walabot", "int", "max", 7, True, 8, {}),
    ("walabot", "u8", "slice_ijk", 7, True, 8, {}),
    ("walabot", "frac", "max", 7, False, 8, {"zoom_rows": 2}),
    ("walabot", "int", "max", 7, True, 8, {"zoom_rows": 1}),
]


@pytest.mark.parametrize("name,kind,mode,mask,scale,B,opts", ROW_CASES,
                         ids=["-".join(str(x) for x in c[:6]) + "".join("-%s%d" % kv for kv in c[6].items()) for c in ROW_CASES])
def test_rows_equal_the_existing_path_and_match_the_reference(rml, rml_opt, name, kind, mode, mask, scale, B, opts):
    src = F.GRIDS[name][0]
    vd, kw, (ref_mode, ref_ijk) = _inputs(rml, name, kind, mode, B)
    z, pm = _zoom(rml, name), _mask(rml, mask)
    # the path that exists: rows at the source grid -> host planes -> process_samples (k_zoom)
    at_source = rml.process_volumes(vd, proj_mask=pm, scale=False, **kw).cpu().numpy()
    want = rml.process_samples(_planes(at_source, src, mask), proj_mask=pm, proj_zoom=z, scale=scale)
    for k, val in opts.items():
        rml_opt(k, val)
    got = rml.process_volumes(vd, proj_mask=pm, scale=scale, proj_zoom=z, **kw).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == (len(at_source), F.feature_len(name, mask))
    np.testing.assert_array_equal(got, want)                    # the same arithmetic: the same bits
    # the reference's own library call on the reference's projections
    ref = F.reference_rows(name, np.array(F.volumes(name, B, kind)), ref_mode, ref_ijk, mask, scale)
    err = np.abs(got.astype(np.float64) - ref).max()
    print("rows vs SciPy: max |diff| = %.3g (bar %.1g)" % (err, ROW_BAR[scale]))
    assert err <= ROW_BAR[scale]


def test_rows_into_a_caller_buffer_and_returned_indices(rml):
    """``out`` with a wider stride keeps its pad columns; ``return_ijk`` hands the derived targets back"""
    import torch
    name, B = "up", 20
    vd, _, _ = _inputs(rml, name, "int", "max", B)
    z = _zoom(rml, name)
    D = F.feature_len(name)
    buf = torch.full((B, D + 5), -7.0, dtype=torch.float32, device="cuda")
    res = rml.process_volumes(vd, scale=True, out=buf, proj_zoom=z)
    assert res is buf and torch.equal(buf[:, :D], rml.process_volumes(vd, scale=True, proj_zoom=z)) and bool((buf[:, D:] == -7.0).all())
    rows, ijk = rml.process_volumes(vd, mode="slice", scale=True, proj_zoom=z, return_ijk=True)
    np.testing.assert_array_equal(ijk.cpu().numpy()[:, 0, :], F.derived_indices(F.volumes(name, B, "int")))
    assert torch.equal(rows, rml.process_volumes(vd, mode="slice", ijk=ijk, scale=True, proj_zoom=z))
    assert torch.equal(rows, rml.process_volumes(vd, mode="slice", scale=True, proj_zoom=z))


# ---- decisions -------------------------------------------------------------------------------------------------------------------------
def _svc(rml, M, name="up", mask=7):
    base = F.reference_rows(name, np.array(F.volumes(name, 64, "int", seed=21)), "max", None, mask, True)
    m = F.synthetic_model(M, F.feature_len(name, mask), base=base)
    svc = rml.GpuSVC(m["sv"], m["dual_coef"], m["intercept"], m["n_support"], m["gamma"], m["classes"], calib_a=m["calib_a"],
                     calib_b=m["calib_b"])
    assert not svc.exact            # a model trained on zoomed rows is off the code grid
    return m, svc


OUTPUTS = ("dec_ovo", "dec_ovr", "label_vote", "proba", "label_calib")


def _check_decisions(rml, m, svc, vd, z, route, bar, **kw):
    import torch
    out = svc.decide_volumes(vd, scale=True, want_proba=True, proj_zoom=z, **kw)
    rows = rml.process_volumes(vd, scale=True, proj_zoom=z, **kw)
    two = dict(zip(("dec_ovo", "dec_ovr", "label_vote", "proba", "label_calib"), svc._decide(rows, want_proba=True)))
    forced = dict(zip(("dec_ovo", "dec_ovr", "label_vote", "proba", "label_calib"), svc._decide(rows, want_proba=True, path=route)))
    for k in OUTPUTS:
        assert torch.equal(out[k], two[k]), k                   # the fused call computes what the two calls compute
        assert torch.equal(out[k], forced[k]), (k, route)       # ... on the kernel the batch size asks for
    ref = F.decision_f64(m, rows.cpu().numpy())
    for k in ("dec_ovo", "dec_ovr", "proba"):
        err = np.abs(out[k].cpu().numpy() - ref[k]).max()
        print("%s vs float64 (%s): max |diff| = %.3g (bar %.1g)" % (k, route, err, bar))
        assert err <= bar, (k, route, err)


@pytest.mark.parametrize("kind,mode,B,opts", [("int", "max", 1, {}), ("frac", "max", 130, {}), ("u8", "max", 300, {}),
                                              ("int", "slice_ijk", 300, {"chunk": 128}), ("u8", "slice_derived", 130, {}),
                                              ("frac", "slice_derived", 300, {"chunk": 128}),
                                              # (one workgroup per row: the norms come from k_zoom_rows itself)
                                              ("frac", "max", 130, {"zoom_rows": 1}), ("u8", "max", 130, {"zoom_rows": 2})],
                         ids=lambda v: str(v).replace(" ", ""))
def test_decisions_equal_rows_plus_decide_float64_route(rml, rml_opt, kind, mode, B, opts):
    m, svc = _svc(rml, 200)
    vd, kw, _ = _inputs(rml, "up", kind, mode, B)
    for k, val in opts.items():
        rml_opt(k, val)
    _check_decisions(rml, m, svc, vd, _zoom(rml, "up"), "f64", BAR_F64, **kw)


def test_decisions_equal_rows_plus_decide_multi_digit_route(rml):
    """A batch over the use_dig_gemm rule of csrc/svm.hip (256 x 256 tiles for at least half a round of one workgroup per CU): the
    zoomed rows go to the multi-digit int8 kernel, in the fused call as in rml_svm_decision."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    M = 1990                                                    # 8 SV tiles of 256
    row_tiles = -(-num_cu // (2 * 8))
    B = (row_tiles - 1) * 256 + 100                             # ragged last tile; 3 940 frames of 22 400 bytes at 256 CUs
    assert -(-B // 256) * 8 * 2 >= num_cu > (-(-300 // 256)) * 1 * 2
    m, svc = _svc(rml, M)
    X, Y, Z = F.GRIDS["up"][0]
    vd, _ = rml.synth_volumes(B, X, Y, Z, seed=77)
    _check_decisions(rml, m, svc, vd, _zoom(rml, "up"), "digits", BAR_DIGITS, mode="max")


def test_several_targets_per_frame_give_frame_major_rows(rml):
    import torch
    m, svc = _svc(rml, 200)
    vd, kw, _ = _inputs(rml, "up", "int", "slice_t2", 9)
    z = _zoom(rml, "up")
    out = svc.decide_volumes(vd, scale=True, proj_zoom=z, **kw)
    assert out["dec_ovo"].shape[0] == 18
    ijk = torch.from_numpy(kw["ijk"]).cuda()
    for t in range(2):
        one = svc.decide_volumes(vd, mode="slice", ijk=ijk[:, t, :], scale=True, proj_zoom=z)
        assert torch.equal(out["dec_ovo"][t::2], one["dec_ovo"]) and torch.equal(out["label_calib"][t::2], one["label_calib"])


# ---- labels against scikit-learn ---------------------------------------------------------------------------------------------------------
def test_svc_labels_equal_scikit_learn_on_scipy_rows(rml):
    import torch
    first, gap = F.sklearn_margins("svc")
    assert first >= F.MARGIN and gap >= F.MARGIN                # a 2e-7 row difference cannot decide a label
    cal, vol, rows = F.sklearn_case("svc")
    est = cal.calibrated_classifiers_[0].estimator
    est = getattr(est, "estimator", est)
    gpu = rml.from_sklearn(cal)
    out = gpu.estimator.decide_volumes(torch.from_numpy(vol).cuda(), mode="max", scale=True, proj_zoom=_zoom(rml, F.SK_GRID))
    np.testing.assert_array_equal(gpu.classes_.take(out["label_vote"].cpu().numpy()), est.predict(rows))
    np.testing.assert_array_equal(gpu.classes_.take(out["label_calib"].cpu().numpy()), cal.predict(rows))
    np.testing.assert_allclose(out["proba"].cpu().numpy(), cal.predict_proba(rows), rtol=0, atol=1e-5)


def test_linear_labels_equal_scikit_learn_on_scipy_rows(rml):
    import torch
    first, gap = F.sklearn_margins("sgd")
    assert first >= F.MARGIN and gap >= F.MARGIN
    cal, vol, rows = F.sklearn_case("sgd")
    est = cal.calibrated_classifiers_[0].estimator
    est = getattr(est, "estimator", est)
    gpu = rml.from_sklearn(cal)
    vd = torch.from_numpy(vol).cuda()
    z = _zoom(rml, F.SK_GRID)
    out = gpu.estimator.decide_volumes(vd, mode="max", scale=True, proj_zoom=z)
    np.testing.assert_array_equal(gpu.classes_.take(out["label"].cpu().numpy()), est.predict(rows))
    np.testing.assert_array_equal(gpu.classes_.take(out["label_calib"].cpu().numpy()), cal.predict(rows))
    # the same scores as the rows + _run composition, bit for bit
    dec = gpu.estimator._run(rml.process_volumes(vd, mode="max", scale=True, proj_zoom=z), want_proba=True)[0]
    assert torch.equal(out["dec"], dec)


# ---- errors, unit zoom, graph capture ------------------------------------------------------------------------------------------------------
def test_a_zoom_that_misses_the_model_raises(rml):
    import torch
    m, svc = _svc(rml, 200)
    lin = rml.GpuLinearClassifier(np.ones((3, F.feature_len("up"))), np.zeros(3), np.arange(3))
    vd = torch.from_numpy(np.array(F.volumes("odd", 4))).cuda()
    for clf in (svc, lin):
        with pytest.raises(ValueError, match="728 features"):
            clf.decide_volumes(vd, proj_zoom=_zoom(rml, "odd"))
        with pytest.raises(ValueError):
            clf.decide_volumes(torch.from_numpy(np.array(F.volumes("up", 4))).cuda(), proj_zoom=_zoom(rml, "down"))
    # the library's own check, both numbers in the message
    import ctypes as C
    from radar_ml_amd import _lib
    arr = (C.c_int32 * 6)(8, 36, 10, 36, 8, 10)
    rc = _lib.load().rml_project_zoom_svm(svc._ctx, svc._h, _lib.ptr(vd), _lib.VOL_F32, 4, 7, 9, 33, _lib.MODE_MAX, None, C.cast(arr, C.c_void_p),
                                          255.0, 7, None, None, None, None, None, _lib.stream_ptr(vd.device))
    msg = _lib.load().rml_last_error().decode()
    assert rc == -1 and "D=728" in msg and "D=1364" in msg, (rc, msg)


def test_an_oversized_plane_is_unsupported(rml):
    import torch
    v = torch.zeros((1, 160, 4, 128), dtype=torch.float32, device="cuda")       # xz: 160 x 128 float64 = 160 KB
    with pytest.raises(rml.RadarMLError, match=r"status -2.*plane too large"):
        rml.process_volumes(v, proj_zoom=rml.ProjZoom(1.1, 1.1, 1.1))
    # the other planes of that arena alone are served
    rows = rml.process_volumes(v, proj_mask=rml.ProjMask(False, True, True), proj_zoom=rml.ProjZoom(1.1, 1.1, 1.1))
    assert rows.shape == (1, 4 * 141 + 176 * 4) and not bool(rows.any())


def test_unit_zoom_is_the_call_without_a_zoom(rml):
    import torch
    name = "up"
    X, Y, Z = F.GRIDS[name][0]
    D = X * Z + Y * Z + X * Y
    m = F.synthetic_model(200, D, seed=3)
    svc = rml.GpuSVC(m["sv"], m["dual_coef"], m["intercept"], m["n_support"], m["gamma"], m["classes"], calib_a=m["calib_a"],
                     calib_b=m["calib_b"])
    lin = rml.GpuLinearClassifier(np.linspace(-1, 1, 3 * D).reshape(3, D), np.zeros(3), np.arange(3))
    one = rml.ProjZoom([1.0, 1.0], [1.0, 1.0], [1.0, 1.0])
    for kind in ("int", "u8"):
        vd, _, _ = _inputs(rml, name, kind, "max", 140)
        want = rml.process_volumes(vd, scale=True)
        for z in (None, one):
            assert torch.equal(rml.process_volumes(vd, scale=True, proj_zoom=z), want)
        for clf in (svc, lin):
            ref = clf.decide_volumes(vd, scale=True)
            for z in (None, one):
                got = clf.decide_volumes(vd, scale=True, proj_zoom=z)
                assert sorted(got) == sorted(ref) and all(torch.equal(got[k], ref[k]) for k in ref), (kind, z)
    feat, q, isum, isq, flags = rml.process_volumes(vd, codes=True, proj_zoom=one)
    assert q is not None and torch.equal(feat, rml.process_volumes(vd))
    with pytest.raises(ValueError):
        rml.process_volumes(vd, codes=True, proj_zoom=_zoom(rml, name))


def test_the_fused_call_captures_into_a_hip_graph(rml):
    """rml_project_zoom_svm after a warm-up (workspace grown) records into a HIP graph -- its second stream and events join the
    capture, as rml_project_svm's do (tests/test_capi_gpu.py) -- and replays on new frames give the eager bits."""
    import torch
    m, svc = _svc(rml, 200)
    z = _zoom(rml, "up")
    X, Y, Z = F.GRIDS["up"][0]
    B = 1000
    Va, _ = rml.synth_volumes(B, X, Y, Z, seed=41)
    Vb, _ = rml.synth_volumes(B, X, Y, Z, seed=43)
    from radar_ml_amd import _lib
    with _lib.options(chunk=256):                                   # four chunks: both workspaces reused
        eager = {}
        for tag, V in (("a", Va), ("b", Vb)):
            o = svc.decide_volumes(V, mode="max", scale=True, want_proba=True, proj_zoom=z)
            eager[tag] = (o["dec_ovo"].clone(), o["label_calib"].clone(), svc.decide_volumes(V[:1], scale=True, proj_zoom=z)["dec_ovo"].clone())
        assert not torch.equal(eager["a"][0], eager["b"][0])
        buf = Va.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                               # the warm-up on the capturing stream (torch's recipe)
            svc.decide_volumes(buf, mode="max", scale=True, want_proba=True, proj_zoom=z)
            svc.decide_volumes(buf[:1], scale=True, proj_zoom=z)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            o = svc.decide_volumes(buf, mode="max", scale=True, want_proba=True, proj_zoom=z)
            o1 = svc.decide_volumes(buf[:1], scale=True, proj_zoom=z)
        for tag, V in (("b", Vb), ("a", Va), ("b", Vb)):
            buf.copy_(V)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(o["dec_ovo"], eager[tag][0]) and torch.equal(o["label_calib"], eager[tag][1]), tag
            assert torch.equal(o1["dec_ovo"], eager[tag][2]), tag
