"""The tie fixtures of tests/svm_ties_common.py are fit to judge a kernel (no GPU): live scikit-learn reproduces the designed pair
values bit for bit, the oracle_np tails equal scikit-learn on every fixture row, every required pattern is present, NO row lies between
an exact tie and a separated row, and a NumPy restatement of csrc/svm_finish.h run with each mutation the suite has to notice changes
at least one output on the fixture (a mutation the fixture cannot see is a missing pattern).

The references use private pieces of scikit-learn (SVC._dual_coef_ .., sklearn.calibration._CalibratedClassifier); where this
scikit-learn lacks one the test skips with that reason -- oracle_np never stands in for it."""
import numpy as np
import pytest

import oracle_np as O
import svm_ties_common as T

CASES = [(C, k) for C in T.CLASS_COUNTS for k in T.KERNELS]


def _live(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except (ImportError, AttributeError) as e:
        pytest.skip("this scikit-learn lacks a private piece the live reference needs: %s" % e)


def _fixtures(C, kernel):
    return [T.fixture(C, kernel), T.fixture(C, kernel, T.VOLUME_D[kernel])]


@pytest.mark.parametrize("C,kernel", CASES)
def test_scikit_learn_reproduces_the_design_and_oracle_np_equals_scikit_learn(C, kernel):
    for fx in _fixtures(C, kernel):
        m = fx.model
        # the design is exact: every weight a multiple of 2^-30, sum |.| below 2^6 -- 36 bits, any order
        W = O.ovo_weight_matrix(m["dual_coef"], m["n_support"])
        for a in (W, m["intercept"]):
            assert np.array_equal(np.rint(a * 2.0 ** 30) * T.TINY, a)
        assert np.abs(W).sum(axis=1).max() + np.abs(m["intercept"]).max() < 64
        assert np.array_equal(fx.dec, T.design_dec(m, fx.codes)) and fx.dec.dtype == np.float64
        assert np.array_equal(fx.X.astype(np.float64), (fx.codes == 255).astype(np.float64))       # on-grid floats are 0.0 and 1.0
        # the oracle's own kernel formulas give the designed kernel values (RBF: exp(-1000 d2) underflows)
        assert np.array_equal(O.svm_kernel_values(fx.X, m["sv"], m["gamma"], kernel), T.design_K(m, fx.codes))
        worst_cal = worst_pw = 0.0
        for name in m["calibs"]:
            ref = _live(T.svc_reference, m, fx.X, name)
            assert np.array_equal(ref.dec_ovo, fx.dec), (fx, "decision_function (ovo)")
            assert np.array_equal(ref.label_vote, O.svm_vote_labels(fx.dec, C)), (fx, "predict")
            ovr = O.sklearn_decision_function(fx.dec, C)
            assert np.array_equal(ref.dec_ovr, ovr) and ref.dec_ovr.shape == ovr.shape, (fx, "decision_function (ovr)")
            pr = O.calibrated_proba(ovr, *m["calibs"][name])
            worst_cal = max(worst_cal, float(np.abs(pr - ref.proba).max()))
            assert np.array_equal(O.calibrated_labels(pr), ref.label_calib), (fx, name)
            pw = O.libsvm_pairwise_proba(fx.dec, m["probA"], m["probB"], C)
            worst_pw = max(worst_pw, float(np.abs(pw - ref.pairwise).max()))
            # the row-by-row restatement (the one the mutations are applied to) is the same function
            r = T.finish_np(fx.dec, C, *m["calibs"][name])
            assert np.array_equal(r.label_vote, ref.label_vote) and np.array_equal(r.dec_ovr, ref.dec_ovr)
            assert np.array_equal(r.label_calib, ref.label_calib) and np.abs(r.proba - ref.proba).max() <= 1e-15
            if name.startswith("sat") and C > 2:
                assert (ref.proba == 1.0 / C).all() and (r.proba == 1.0 / C).all() and (ref.label_calib == 0).all()
        print("%r: %d rows, |calibrated - sklearn| %.2e, |pairwise - sklearn| %.2e" % (fx, fx.N, worst_cal, worst_pw))
        assert worst_cal <= 1e-15 and worst_pw <= 1e-15


@pytest.mark.parametrize("C,kernel", CASES)
def test_every_required_pattern_is_present_and_no_row_lies_in_between(C, kernel):
    for fx in _fixtures(C, kernel):
        m = fx.model
        need = T.required(C, kernel)
        have = {k: int(fx.pat[k].sum()) for k in need}
        print("%r: %d rows (%d edge, %d fit float32) %s" % (fx, fx.N, fx.edge.sum(), fx.f32_ok.sum(), have))
        assert not fx.short, fx.short
        for k, n in need.items():
            assert have[k] >= n, (fx, k, have[k], n)
        assert fx.N <= T.N_BATCH and len(m["codes"]) <= 18 and fx.D <= 160
        # a condition, not a measurement: the cap on rows in between is zero
        a = np.abs(fx.dec)
        assert ((a == 0.0) | (a >= 2.0 ** -31)).all()
        assert not fx.between.any()
        ovr = O.sklearn_decision_function(fx.dec, C)
        for name in ("equal", "unequal"):
            gap = T._top_gap(O.calibrated_proba(ovr, *m["calibs"][name]))
            assert ((gap == 0.0) | (gap >= T.GAP)).all(), (fx, name)
            if name == "unequal":
                assert (gap >= T.GAP).all()
        if C == 2:
            z = fx.dec[:, 0] == 0.0
            assert z.any() and np.signbit(ovr[z]).all()                                              # T = -0.0
            ref = _live(T.svc_reference, m, fx.X[z], "equal", proba=False)
            assert (ref.proba == 0.5).all() and (ref.label_calib == 0).all() and (ref.label_vote == 1).all()
        # controls sit between the edge rows, and the batch puts an edge row on every tile boundary
        idx = fx.batch()
        assert len(idx) == T.N_BATCH and fx.edge[idx[list(T.EDGE_POSITIONS)]].all() and set(idx) == set(range(fx.N))
        # the float32 subset is worked out per row; a value that needs more than 24 bits is never in it
        assert 0 < fx.f32_ok.sum()
        assert np.array_equal(fx.dec[fx.f32_ok].astype(np.float32).astype(np.float64), fx.dec[fx.f32_ok])


@pytest.mark.parametrize("C,kernel", CASES)
def test_volume_fixtures_hold_ties_and_nothing_in_between(C, kernel):
    """the frames tests/test_svm_ties_gpu.py feeds the fused front doors: features 0 / 1 by the oracle's projection, live scikit-learn
    on them gives the designed values"""
    for mode in ("max", "slice"):
        v = T.volume_fixture(C, kernel, mode)
        assert v.vol.shape[1:] == T.GRID and set(np.unique(v.vol)) <= {0, 255} and v.N <= T.N_BATCH
        assert not v.between.any() and (v.dec == 0.0).any() and v.pat["control"].sum() >= 10
        if kernel == "linear":
            assert v.pat["proba_tie"].any() and (C == 2 or any(v.pat[k].any() for k in T.reachable_vote_ties(C)))
        ref = _live(T.svc_reference, v.model, v.X, "equal", proba=False)
        assert np.array_equal(ref.dec_ovo, v.dec)


def test_which_vote_ties_exist():
    assert T.reachable_vote_ties(3) == ("vote_cycle", "vote_tie_all")                       # two tied at the top tie the third
    assert "vote_tie_all" not in T.reachable_vote_ties(4) and "vote_tie_all" not in T.reachable_vote_ties(6)
    assert set(T.reachable_vote_ties(5)) == {"vote_cycle", "vote_tie_all", "vote_tie_top_with_0", "vote_tie_top_without_0"}


@pytest.mark.parametrize("C", T.CLASS_COUNTS)
def test_every_mutation_of_the_finish_changes_the_fixture(C):
    """teeth: each rule of k_svm_finish, flipped, shows on some row of the linear fixture of this C"""
    fx = T.fixture(C, "linear")
    m = fx.model
    flags = np.ones(fx.N, np.int32)
    flags[[1, fx.N // 2]] = 0
    seen = {}
    for mut in T.MUTATIONS:
        if mut in T.UNREACHABLE:
            continue                                    # pr > 1 cannot be produced: svm_ties_common's docstring has the argument
        changed = 0
        for name in m["calibs"]:
            good = T.finish_np(fx.dec, C, *m["calibs"][name], flags=flags)
            bad = T.finish_np(fx.dec, C, *m["calibs"][name], flags=flags, mut=mut)
            for k in ("dec_ovr", "proba", "label_vote", "label_calib"):
                x, y = getattr(good, k), getattr(bad, k)
                changed += int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum())
        seen[mut] = changed
    print("ties-C%d finish mutations -> changed outputs %s" % (C, seen))
    expect = set(T.MUTATIONS) - set(T.UNREACHABLE)
    if C == 2:
        # one pair: no vote tie and no arg-max tie beyond (0.5, 0.5), where the first maximum is also what ">" keeps; the binary tail
        # has no denominator.  The rules below are the ones two classes have
        expect = {"vote_ge", "proba_last_max", "invalid_not_marked"}
    for mut in expect:
        assert seen[mut] > 0, (C, mut)


def test_the_clamp_is_unreachable():
    """pr > 1 needs fl(x / fl(x + rest)) > 1 with rest >= 0: never (monotone rounding).  Tried on the values closest to it."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.random(20000), 1.0 - 2.0 ** -rng.integers(1, 54, 20000), [1.0, 0.5, 2.0 ** -1074]])
    for rest in (0.0, 2.0 ** -1074, 2.0 ** -60, 1e-17):
        assert (x / (x + rest) <= 1.0).all()
    assert (1.0 - x <= 1.0).all()
    for C in (3, 6):
        fx = T.fixture(C, "linear")
        for name, cal in fx.model["calibs"].items():
            assert O.calibrated_proba(O.sklearn_decision_function(fx.dec, C), *cal).max() <= 1.0


@pytest.mark.parametrize("C", T.CLASS_COUNTS)
def test_pairwise_fixture_clips_both_ends_and_its_mutations_show(C):
    fx = T.fixture(C, "linear")
    m = fx.model
    f = fx.dec * m["probA"] + m["probB"]
    lo, hi = int((f < -17).any(1).sum()), int((f > 17).any(1).sum())
    good, iters = T.pairwise_np(fx.dec, m["probA"], m["probB"], C)
    assert np.array_equal(good, O.libsvm_pairwise_proba(fx.dec, m["probA"], m["probB"], C))
    cap = max(100, C)
    capped = int((iters >= cap).sum())
    print("ties-C%d pairwise: %d rows clip at 1e-7, %d at 1 - 1e-7; iterations max %d, rows at the cap %d of %d"
          % (C, hi, lo, iters.max(), capped, fx.N))
    assert lo >= 1 and hi >= 1
    assert not np.array_equal(T.pairwise_np(fx.dec, m["probA"], m["probB"], C, mut="no_clip")[0], good)
    # a row that does not converge before the cap: searched, none exists.  Candidates: the fixture rows, and 600 rows of pair values
    # from {-1, 1, 0, 0.03, 0.3} under sigmoids steep in EVERY pair (A = -32: clipped at both ends, cycles included).  With r clipped
    # to [1e-7, 1 - 1e-7] and the loose stopping rule (eps = 0.005 / k) libsvm's iteration stops after at most five sweeps, so no
    # cap of five or more can be told from 100 by any row; a cap below the sweeps a row needs is seen
    P = C * (C - 1) // 2
    rng = np.random.default_rng(C)
    extreme = rng.choice([-1.0, 1.0, 0.0, 0.03, 0.3], (600, P))
    far, it2 = T.pairwise_np(extreme, np.full(P, -32.0), np.zeros(P), C)
    most = int(max(iters.max(), it2.max()))
    print("ties-C%d pairwise: most sweeps over %d candidates: %d (cap %d)" % (C, fx.N + len(extreme), most, cap))
    assert capped == 0 and most <= 5
    if C > 2:
        short = T.pairwise_np(fx.dec, m["probA"], m["probB"], C, cap=int(iters.max()) - 1)[0]
        assert not np.array_equal(short, good)


@pytest.mark.parametrize("C", T.CLASS_COUNTS)
@pytest.mark.parametrize("D", T.LINEAR_D)
def test_linear_classifier_fixture(C, D):
    fx = T.linear_fixture(C, D)
    have = {k: int(v.sum()) for k, v in fx.pat.items()}
    print("%r: %d rows %s" % (fx, fx.N, have))
    for k, n in fx.need().items():
        assert have[k] >= n, (fx, k)
    assert not fx.between.any() and fx.N <= T.N_BATCH
    assert set(np.unique(fx.X)) <= {0.0, 1.0}
    for a in (fx.coef, fx.intercept):
        assert np.array_equal(np.rint(a * 16) / 16, a)
    seen = {mut: 0 for mut in T.LINEAR_MUTATIONS}
    for name, cal in fx.calibs.items():
        ref = _live(T.linear_reference, fx, name)
        want = fx.scores[:, 0] if C == 2 else fx.scores
        assert np.array_equal(ref.dec, want) and ref.dec.shape == want.shape
        r = T.linear_np(fx.X, fx.coef, fx.intercept, C, *cal)
        assert np.array_equal(r.dec, ref.dec) and np.array_equal(r.label, ref.label)
        assert np.array_equal(r.label_calib, ref.label_calib) and np.abs(r.proba - ref.proba).max() <= 1e-15
        assert np.abs(O.calibrated_proba(ref.dec, *cal) - ref.proba).max() <= 1e-15
        gap = T._top_gap(ref.proba)
        assert ((gap == 0.0) | (gap >= T.GAP)).all()
        for mut in T.LINEAR_MUTATIONS:
            bad = T.linear_np(fx.X, fx.coef, fx.intercept, C, *cal, mut=mut)
            for k in ("label", "proba", "label_calib"):
                x, y = getattr(r, k), getattr(bad, k)
                seen[mut] += int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum())
    expect = {"bin_score_ge", "bin_proba_ge"} if C == 2 else {"label_last_max", "proba_last_max", "no_uniform"}
    print("%r mutations -> changed outputs %s" % (fx, seen))
    for mut in expect:
        assert seen[mut] > 0, (fx, mut)
