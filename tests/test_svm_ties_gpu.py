"""csrc/svm_finish.h at exact ties and exact saturation, against LIVE scikit-learn (tests/svm_ties_common.py builds the fixtures,
tests/test_svm_ties_cpu.py shows they are fit to judge).

Every decision value of a fixture is a short sum of dyadic numbers: exact in float64 whatever the order, so every path must return the
DESIGNED bits, and then the vote at dec == 0, the first maximum among tied votes and tied probabilities, the uniform fallback and
the NaN / -1 marks of invalid rows are rules, compared with SVC.predict, SVC.decision_function, _CalibratedClassifier.predict_proba,
SVC.predict_proba and SGDClassifier of the installed scikit-learn -- never with stored arrays, and never with oracle_np in their
place (a private piece missing from this scikit-learn skips the test with that reason).

Bars: dec_ovo, dec_ovr and the linear scores bit for bit (==, so -0.0 equals 0.0); labels equal on every row (the fixtures hold exact
ties and separated rows only); proba within PROBA_BAR = 1e-9 max(1, max |dec|), the bar tests/test_svm_geometry_gpu.py applies to the
exact routes (device exp against libm, an fma in a T + b), tied entries bit-equal, saturated rows exactly 1 / C; the pairwise
probabilities within TOL of tests/test_svm_gpu.py.  The float32 path gets the rows whose sums fit 24 bits (fixture.f32_ok).

The multi-digit path: the frame of a one-hot model is s = 1 (hi - lo = 1 is a power of two: csrc/svm.hip, "an exact power of two is its
own scale"), c0 = 1/2, so features 0 and 1 are the fixed-point digits -+2^30 and squared distances are the integers 0, 1, 2: the
path reproduces the design bit for bit like the others and is held to the same assertions (no path needed the weaker bar).

One "TIES" line per run: case, path, entry, rows, zero pairs, vote ties, probability ties, max |proba - ref|; run with -s."""
import types

import numpy as np
import pytest
import torch

import oracle_np as O
import svm_geometry_common as G
import svm_ties_common as T
from test_svm_geometry_gpu import KEYS, _code_operand, _decide, _has_digit_frame, _host, _svc
from test_svm_gpu import TOL

pytestmark = pytest.mark.gpu

CASES = [(C, k) for C in T.CLASS_COUNTS for k in T.KERNELS]
ROUND_OFF = 1e-9            # the bar of the exact routes in tests/test_svm_geometry_gpu.py at |dec| <= 1
_refs = {}


def _reference(key, model, X, calib):
    """live scikit-learn on the rows of a fixture, once per (fixture, calibrators); shared and never written to"""
    k = (key, calib)
    if k not in _refs:
        try:
            _refs[k] = T.svc_reference(model, X, calib, proba=False)
        except (ImportError, AttributeError) as e:
            pytest.skip("this scikit-learn lacks a private piece the live reference needs: %s" % e)
    return _refs[k]


def _take(ref, idx):
    return types.SimpleNamespace(**{k: v[idx] for k, v in vars(ref).items()})


def _with_calib(model, name):
    m = dict(model)
    m["calib_a"], m["calib_b"] = model["calibs"][name]
    return m


def _judge(tag, got, ref, dec, C):
    """every assertion of one run; ``dec`` the designed pair values of its rows"""
    n = len(dec)
    assert got.dec_ovo.shape == dec.shape and got.proba.shape == (n, C)
    assert (got.dec_ovo == dec).all(), (tag, "dec_ovo", np.abs(got.dec_ovo - dec).max())
    assert np.array_equal(got.label_vote, ref.label_vote), (tag, "label_vote", np.flatnonzero(got.label_vote != ref.label_vote))
    assert got.dec_ovr.shape == ref.dec_ovr.shape and (got.dec_ovr == ref.dec_ovr).all(), (tag, "dec_ovr")
    assert np.array_equal(got.label_calib, ref.label_calib), (tag, "label_calib", np.flatnonzero(got.label_calib != ref.label_calib))
    err = float(np.abs(got.proba - ref.proba).max())
    bar = 1e-9 * max(1.0, float(np.abs(dec).max()))
    top = np.sort(ref.proba, axis=1)
    tie = top[:, -1] == top[:, -2]
    mine = np.sort(got.proba, axis=1)
    assert (mine[tie, -1] == mine[tie, -2]).all(), (tag, "tied probabilities differ")
    uniform = (ref.proba == 1.0 / C).all(axis=1)
    assert (got.proba[uniform] == 1.0 / C).all(), (tag, "uniform rows")
    v = T.votes_of(dec, C)
    vote_ties = int(((v == v.max(1, keepdims=True)).sum(1) >= 2).sum())
    print("TIES %s rows=%d zero_pairs=%d vote_ties=%d proba_ties=%d max|proba-ref|=%.2e (bar %.1e)"
          % (tag, n, int((dec == 0.0).sum()), vote_ties, int(tie.sum()), err, bar))
    assert err <= bar, (tag, err)


def _paths_of(rml, svc, fx):
    """(path, rows of the fixture it gets); a model without a digit frame refuses the digit path cleanly"""
    out = []
    for path in T.PATHS:
        if path == "digits" and not _has_digit_frame(fx.model):
            with pytest.raises(rml.RadarMLError, match="no digit frame"):
                svc._decide(svc._rows(fx.X), path="digits")
            continue
        out.append((path, np.flatnonzero(fx.f32_ok) if path == "f32" else np.arange(fx.N)))
    return out


# ---- GpuSVC._decide: a batch of 300 and single observations ------------------------------------------------------------------------------
@pytest.mark.parametrize("C,kernel", CASES)
def test_decide_batch_of_300_on_every_path(rml, C, kernel):
    """edge rows at 0, 63, 64, 127, 128, 129, 255, 256 and 299 with controls between them; every calibrator set on the auto path (the
    finish kernel is the same behind every GEMM), the equal calibrators on all of them"""
    fx = T.fixture(C, kernel)
    ref = _reference(repr(fx), fx.model, fx.X, "equal")
    svc = _svc(rml, fx.model)
    batch = fx.batch()
    for path, rows in _paths_of(rml, svc, fx):
        idx = batch[np.isin(batch, rows)]
        _judge("%r %s batch" % (fx, path), _decide(svc, fx.X[idx], path), _take(ref, idx), fx.dec[idx], C)
    for name in ("unequal", "sat0", "sat1"):
        other = _svc(rml, _with_calib(fx.model, name))
        r = _reference(repr(fx), fx.model, fx.X, name)
        got = _decide(other, fx.X[batch], "auto")
        _judge("%r auto batch calib=%s" % (fx, name), got, _take(r, batch), fx.dec[batch], C)
        if name != "unequal" and C > 2:
            assert (got.proba == 1.0 / C).all() and (got.label_calib == 0).all()          # den == 0 (sat0) and every sigmoid 1 (sat1)


@pytest.mark.parametrize("C,kernel", CASES)
def test_decide_single_observations(rml, C, kernel):
    """N = 1 (the matrix-vector kernels of svm_small.h on the exact paths): one row of every pattern and four controls, one call each"""
    fx = T.fixture(C, kernel)
    ref = _reference(repr(fx), fx.model, fx.X, "equal")
    svc = _svc(rml, fx.model)
    for path, rows in _paths_of(rml, svc, fx):
        edge = []
        for name in sorted(fx.pat):                      # the first row of every pattern this path gets
            hit = [i for i in rows if fx.pat[name][i] and name != "control"]
            if hit and hit[0] not in edge:
                edge.append(hit[0])
        ctrl = [i for i in rows if not fx.edge[i]][:4]
        idx = np.array(edge + ctrl)
        parts = [_decide(svc, fx.X[i:i + 1], path) for i in idx]
        got = types.SimpleNamespace(**{k: np.concatenate([getattr(p, k) for p in parts]) for k in KEYS})
        _judge("%r %s N=1" % (fx, path), got, _take(ref, idx), fx.dec[idx], C)


# ---- decide_codes: code rows, with and without row flags ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,kernel", CASES)
def test_decide_codes_and_invalid_rows(rml, C, kernel):
    """forced int8 on uint8 codes: a row flagged invalid is label_vote == label_calib == -1 and NaN in dec_ovo, dec_ovr and proba; the
    valid rows beside it keep their bits"""
    fx = T.fixture(C, kernel)
    ref = _reference(repr(fx), fx.model, fx.X, "equal")
    svc = _svc(rml, fx.model)
    batch = fx.batch()
    q, isum, isq = _code_operand(fx.codes[batch])
    plain = _host(svc.decide_codes(q, isum, isq, None, want_proba=True))
    _judge("%r codes" % fx, plain, _take(ref, batch), fx.dec[batch], C)
    ones = torch.ones(len(batch), dtype=torch.int32, device=q.device)
    allvalid = _host(svc.decide_codes(q, isum, isq, ones, want_proba=True))
    for k in KEYS:
        assert np.array_equal(getattr(allvalid, k), getattr(plain, k)), k
    bad = np.array([0, 1, 64, 127, 128, 200, 299])
    flags = np.ones(len(batch), np.int32)
    flags[bad] = 0
    got = _host(svc.decide_codes(q, isum, isq, torch.from_numpy(flags).cuda(), want_proba=True))
    assert (got.label_vote[bad] == -1).all() and (got.label_calib[bad] == -1).all()
    for k in ("dec_ovo", "dec_ovr", "proba"):
        assert np.isnan(getattr(got, k)[bad]).all(), k
    ok = flags != 0
    for k in KEYS:
        assert np.array_equal(getattr(got, k)[ok], getattr(plain, k)[ok]), k
    print("TIES %r codes with flags: %d invalid rows NaN / -1, %d valid rows keep their bits" % (fx, len(bad), int(ok.sum())))


# ---- decide_volumes: the fused front doors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "slice"])
@pytest.mark.parametrize("C,kernel", CASES)
def test_decide_volumes_on_a_4x4x8_grid(rml, C, kernel, mode):
    """voxels 0 or 255 (features 0 or 1 after scaling), as float32 and as uint8 volumes; max mode and slices at given (i, j, k); the
    unit zoom takes the same call; without ijk the slices go through the frame's derived target (rml_derive_project_svm where the
    shape has the fused kernel, derive_targets + rml_project_svm otherwise): the features of THOSE indices by the oracle's
    projection go to the same live references"""
    v = T.volume_fixture(C, kernel, mode)
    m = v.model
    mask = rml.ProjMask(*v.mask)
    assert rml.feature_len(*T.GRID, mask) == v.codes.shape[1]
    ref = _reference(repr(v), m, v.X, "equal")
    svc = _svc(rml, m)
    kw = dict(mode=mode, proj_mask=mask, scale=True)
    if mode == "slice":
        kw["ijk"] = v.ijk
    outs = {}
    for name, vol in (("f32", torch.from_numpy(v.vol.astype(np.float32)).cuda()), ("u8", torch.from_numpy(v.vol).cuda())):
        o = svc.decide_volumes(vol, **kw)
        torch.cuda.synchronize()
        outs[name] = types.SimpleNamespace(**{k: o[k].cpu().numpy() for k in KEYS})
        _judge("%r volumes %s" % (v, name), outs[name], ref, v.dec, C)
    for k in KEYS:
        assert np.array_equal(getattr(outs["u8"], k), getattr(outs["f32"], k)), k
    unit = rml.ProjZoom(xz=[1.0, 1.0], yz=[1.0, 1.0], xy=[1.0, 1.0])
    o = svc.decide_volumes(torch.from_numpy(v.vol).cuda(), proj_zoom=unit, **kw)
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(o[k].cpu().numpy(), getattr(outs["u8"], k)), ("unit zoom", k)
    if mode == "slice":
        vol = torch.from_numpy(v.vol).cuda()
        o = svc.decide_volumes(vol, mode="slice", proj_mask=mask, scale=True)
        torch.cuda.synchronize()
        ijk = (o["ijk"] if "ijk" in o else rml.derive_targets(vol, 1)[:, 0, :]).cpu().numpy()
        codes = T.volume_codes(v.vol, "slice", ijk, v.mask)
        if kernel == "rbf":
            keep = (codes == 255).sum(1) <= 1                        # one voxel per frame: always
            assert keep.all()
        X = G.on_grid(codes)
        dref = T.svc_reference(m, X, "equal", proba=False)
        dec = T.design_dec(m, codes)
        assert np.array_equal(dref.dec_ovo, dec)
        # these frames were chosen for the GIVEN indices; at the derived ones a row may lie in between: judged are the others
        keep = ~T.patterns_of(dec, C, m["calibs"])[1]
        got = types.SimpleNamespace(**{k: o[k].cpu().numpy()[keep] for k in KEYS})
        _judge("%r volumes derived (%s, %d of %d rows)" % (v, "fused" if "ijk" in o else "two calls", int(keep.sum()), len(keep)),
               got, _take(dref, keep), dec[keep], C)


# ---- the null model: dec = intercept for any row --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,kernel", CASES)
def test_null_model_on_random_rows(rml, C, kernel):
    """dual coefficients all zero (rml_svm_load takes the model): dec == intercept on rows OFF the code grid, which reach the float64,
    float32 and multi-digit GEMMs with arbitrary kernel values; the forced int8 path gets the rows on the grid (off it, it marks them
    invalid).  The intercept holds a zero, +-2^-30 and multiples of 1/16."""
    m = T.null_model(C, kernel)
    rng = np.random.default_rng([C, 11])
    N = 150
    codes = G.draw_codes(rng, (N, m["sv"].shape[1]))
    Xon = G.on_grid(codes)
    Xoff = (rng.random(Xon.shape, dtype=np.float32) * np.float32(0.97)).astype(np.float32)
    dec = np.broadcast_to(m["intercept"], (N, len(m["intercept"]))).copy()
    assert (dec == 0.0).any()
    svc = _svc(rml, m)
    for path in T.PATHS:
        if path == "digits" and not _has_digit_frame(m):
            continue
        X = Xon if path == "i8" else Xoff
        ref = _reference(("null", C, kernel, path == "i8"), m, X, "equal")
        assert np.array_equal(ref.dec_ovo, dec)
        _judge("null-C%d-%s %s" % (C, kernel, path), _decide(svc, X, path), ref, dec, C)
        _judge("null-C%d-%s %s N=1" % (C, kernel, path), _decide(svc, X[:1], path), _take(ref, slice(0, 1)), dec[:1], C)


# ---- rml_svm_pairwise_proba -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,kernel", CASES)
def test_pairwise_proba_against_live_predict_proba(rml, C, kernel):
    """SVC.predict_proba of the bare SVC (k_pairwise_proba) with a steep first pair: rows beyond |dec A + B| = 17 sit on the 1e-7 clip,
    at both ends; the bar is the one of test_svm_gpu.py's Platt test"""
    fx = T.fixture(C, kernel)
    m = fx.model
    try:
        ref = T.svc_reference(m, fx.X, "equal").pairwise
    except (ImportError, AttributeError) as e:
        pytest.skip("this scikit-learn lacks a private piece the live reference needs: %s" % e)
    svc = rml.GpuSVC(m["sv"], m["dual_coef"], m["intercept"], m["n_support"], m["gamma"], m["classes"], kernel=kernel,
                     probA=m["probA"], probB=m["probB"])
    got = svc.predict_proba(fx.X)
    f = fx.dec * m["probA"] + m["probB"]
    clip = (np.abs(f) > 17).any(axis=1)
    err = float(np.abs(got - ref).max())
    print("TIES %r pairwise rows=%d clip rows=%d max|proba-ref|=%.2e (clip rows %.2e; bar %.0e)"
          % (fx, fx.N, int(clip.sum()), err, float(np.abs(got - ref)[clip].max()) if clip.any() else 0.0, TOL))
    assert got.shape == ref.shape and err <= TOL
    # ... and, since the pair values going in are bit-equal here and both sides run libsvm's float64 operations in libsvm's order (what
    # differs is exp: the device routine against libm, an ulp or so), within the float64 round-off bar of the exact routes as well.
    # Without it the 1e-7 clip has no teeth: dropping the clip moves these probabilities by 3e-8 .. 1e-7, far inside TOL
    assert err <= ROUND_OFF, err
    if kernel == "linear":
        assert (f > 17).any() and (f < -17).any()
    one = svc.predict_proba(fx.X[:1])
    assert np.array_equal(one, got[:1])


# ---- k_linear -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", T.LINEAR_D)
@pytest.mark.parametrize("C", T.CLASS_COUNTS)
def test_linear_classifier_ties(rml, C, D):
    """GpuLinearClassifier on dyadic coefficients and binary rows, D across the 64 lanes of a wave (a lane owns nothing, one element,
    two): scores bit-equal to SGDClassifier.decision_function, predict equal (score 0 is class 0 of two; the first of tied scores),
    the calibrated tail as for the SVC"""
    fx = T.linear_fixture(C, D)
    for name, (a, b) in fx.calibs.items():
        try:
            ref = T.linear_reference(fx, name)
        except (ImportError, AttributeError) as e:
            pytest.skip("this scikit-learn lacks a private piece the live reference needs: %s" % e)
        clf = rml.GpuLinearClassifier(fx.coef, fx.intercept, np.arange(C), a, b)
        runs = [("batch", np.arange(fx.N))] + ([("N=1", np.arange(min(fx.N, 8)))] if name == "equal" else [])
        for what, idx in runs:
            if what == "batch":
                dec, lab, proba, labc = [t.cpu().numpy() for t in clf._run(clf._rows(fx.X), want_proba=True)]
            else:
                parts = [[t.cpu().numpy() for t in clf._run(clf._rows(fx.X[i:i + 1]), want_proba=True)] for i in idx]
                dec, lab, proba, labc = [np.concatenate([p[j] for p in parts]) for j in range(4)]
            assert dec.shape == ref.dec[idx].shape and (dec == ref.dec[idx]).all(), (fx, name, what)
            assert np.array_equal(lab, ref.label[idx]) and np.array_equal(labc, ref.label_calib[idx]), (fx, name, what)
            err = float(np.abs(proba - ref.proba[idx]).max())
            top, mine = np.sort(ref.proba[idx], axis=1), np.sort(proba, axis=1)
            tie = top[:, -1] == top[:, -2]
            assert (mine[tie, -1] == mine[tie, -2]).all()
            if name.startswith("sat") and C > 2:
                assert (proba == 1.0 / C).all() and (labc == 0).all()
            scores = fx.scores[idx]
            top_s = (scores == scores.max(1, keepdims=True)).sum(1) >= 2 if C > 2 else scores[:, 0] == 0.0
            print("TIES %r calib=%s %s rows=%d zero_scores=%d score_ties=%d proba_ties=%d max|proba-ref|=%.2e"
                  % (fx, name, what, len(idx), int((scores == 0.0).sum()), int(top_s.sum()), int(tie.sum()), err))
            assert err <= 1e-9 * max(1.0, float(np.abs(scores).max()))
        assert np.array_equal(clf.predict(fx.X), ref.label) and (clf.decision_function(fx.X) == ref.dec).all()


# ---- the finish is consistent with its own pair values on the geometry cases ----------------------------------------------------------------
SELF_CASES = [(G.BASE["M"], G.BASE["D"], Cn, G.BASE["N"], p, "rbf") for Cn, p in G.C_AXIS] + \
             [(G.BASE["M"], G.BASE["D"], G.BASE["C"], G.BASE["N"], "balanced", "linear")]


@pytest.mark.parametrize("key", SELF_CASES, ids=lambda k: "M%d-D%d-C%d-N%d-%s-%s" % k)
def test_tails_follow_from_the_returned_pair_values(rml, key):
    """the rows the geometry sweep's label checks leave out: given the dec_ovo the device returned, label_vote is the libsvm vote on
    EVERY row, dec_ovr is oracle_np's bit for bit, and label_calib is the arg-max of the recomputed probabilities except where their
    top-2 gap is below 1e-12 (counted, and capped by the 1 % near-tie cap tests/test_svm_geometry_cpu.py holds the case to)"""
    c = G.case(*key)
    Cn = c.C
    svc = _svc(rml, c.model)
    for path in G.PATHS:
        if path == "digits" and not _has_digit_frame(c.model):
            continue
        got = _decide(svc, c.X if path in ("auto", "i8") else c.Xoff, path)
        assert np.array_equal(got.label_vote, O.svm_vote_labels(got.dec_ovo, Cn)), (c, path)
        ovr = O.sklearn_decision_function(got.dec_ovo, Cn)
        assert got.dec_ovr.shape == ovr.shape and (got.dec_ovr == ovr).all(), (c, path, np.abs(got.dec_ovr - ovr).max())
        pr = O.calibrated_proba(ovr, c.model["calib_a"], c.model["calib_b"])
        top = np.sort(pr, axis=1)
        close = (top[:, -1] - top[:, -2]) < 1e-12
        print("TIES %r %s self-consistency: %d rows, %d with a recomputed top-2 gap below 1e-12" % (c, path, c.N, int(close.sum())))
        assert close.sum() <= 0.01 * c.N
        assert np.array_equal(got.label_calib[~close], O.calibrated_labels(pr)[~close]), (c, path)
