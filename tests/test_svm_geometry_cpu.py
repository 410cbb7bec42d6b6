"""Self-check of the synthetic SVC cases of tests/svm_geometry_common.py, on the references alone (no GPU): a case can only judge a
kernel if its rows are not near-ties, its kernel values are spread, and its two references agree to the input-rounding floor.
One line per case: near-tie counts (expected 0) and the floor between the two references."""
import numpy as np
import pytest

import svm_geometry_common as G
from test_svm_gpu import _tol               # the project's relative bar of the linear kernel (nothing of that module runs here)

KEYS = G.all_case_keys()


def _batches(c):
    """the case itself, and for the N axis every smaller batch (its first rows)"""
    if c.N == G.N_MAX and c.D in G.N_AXIS_D and (c.M, c.C, c.pattern) == (G.BASE["M"], G.BASE["C"], "balanced"):
        return [c.first(n) for n in G.N_AXIS]
    return [c]


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "M%d-D%d-C%d-N%d-%s-%s" % k)
def test_generated_case_is_fit_to_judge_a_kernel(key):
    M, D, C, N, pattern, kernel = key
    c = G.case(*key)
    m = c.model
    assert int(m["n_support"].sum()) == M and len(m["n_support"]) == C and (m["n_support"] >= 0).all()
    assert m["dual_coef"].shape == (C - 1, M) and np.abs(m["dual_coef"]).max() <= 1.0 and M <= 385       # sum |w| <= 385
    assert np.array_equal(c.codes[0], m["codes"][0])                                                  # row 0 is SV 0
    assert np.array_equal((m["sv"] * 255.0).round().astype(np.uint8), m["codes"])
    assert np.array_equal(m["sv"].astype(np.float32).astype(np.float64), m["sv"])                    # float32-representable
    ex, fr = c.exact, c.f32
    if kernel == "rbf":
        assert ex.K[0, 0] == 1.0
        if D >= 31 and N >= 8:
            # the spread the generator is built for: each row against its nearest SV (the one it was copied from).  Over ALL (row, SV)
            # entries the range cannot be asked for: distances between unrelated sparse rows concentrate as D grows (D = 255: the
            # 10 %-90 % range of the whole matrix is 0.33..0.40 around the median e^-1 that gamma sets), whatever the rows are
            q10, q90 = np.quantile(ex.K.max(axis=1), [0.1, 0.9])
            assert q90 - q10 > 0.1, (q10, q90)
    # the two references differ by the rounding of float32(c / 255) alone
    floor = float(np.abs(ex.dec_ovo - fr.dec_ovo).max())
    bar = 1e-6 if kernel == "rbf" else _tol(m, fr.dec_ovo)
    kfloor = float(np.abs(ex.K - fr.K).max())
    for b in _batches(c):
        pair, gap = G.margins(b.exact)
        ties_pair, ties_gap = int((pair < G.NEAR_TIE).sum()), int((gap < G.NEAR_TIE).sum())
        pair_f, gap_f = G.margins(b.f32)
        ties_pair = max(ties_pair, int((pair_f < G.NEAR_TIE).sum()))
        ties_gap = max(ties_gap, int((gap_f < G.NEAR_TIE).sum()))
        print("%r: near-ties pair %d gap %d of %d rows (min |pair| %.2e, min gap %.2e); |ref_exact - ref_f32rows| dec %.2e K %.2e"
              % (b, ties_pair, ties_gap, b.N, pair.min(), gap.min(), floor, kfloor))
        assert ties_pair <= 0.01 * b.N and ties_gap <= 0.01 * b.N
        # ... and at the widest margin the GPU sweep excludes rows at under the same cap (ten times the bar of the digit route), on the
        # rows the float routes are given
        wide = [int(((p < G.CAP_MARGIN) | (g < G.CAP_MARGIN)).sum()) for p, g in (G.margins(b.exact), G.margins(b.f32off))]
        assert max(wide) <= 0.01 * b.N, wide
    assert floor <= bar, floor
    assert np.abs(ex.dec_ovr - fr.dec_ovr).max() <= bar and np.abs(ex.proba - fr.proba).max() <= bar
    assert np.array_equal(ex.label_vote, fr.label_vote) and np.array_equal(ex.label_calib, fr.label_calib)


def test_n_support_patterns():
    assert list(G.n_support_of(129, 3, "balanced")) == [43, 43, 43]
    assert list(G.n_support_of(7, 3, "balanced")) == [3, 2, 2]
    assert list(G.n_support_of(1, 3, "balanced")) == [1, 0, 0]
    assert list(G.n_support_of(129, 4, "single")) == [1, 43, 43, 42]
    assert list(G.n_support_of(129, 3, "empty")) == [65, 64, 0]
    assert not G.pattern_allowed(2, 3, "single") and not G.pattern_allowed(129, 2, "empty")


def test_gamma_puts_the_median_kernel_value_at_one_over_e():
    c = G.case(129, 129, 3, 129)
    d2 = G.code_sq_distances(c.codes, c.model["codes"])
    med = np.median(np.exp(-c.model["gamma"] * d2[d2 > 0] / 65025.0))
    assert abs(med - np.exp(-1.0)) < 0.05, med            # gamma comes from a probe batch of the same generator, not from these rows
    assert G.gamma_for(np.zeros((3, 1), np.uint8), np.zeros((2, 1), np.uint8)) == 1.0


def test_rows_leave_the_code_grid_when_scaled():
    c = G.case(129, 129, 3, 129)
    back = np.rint(c.Xoff * G.F255).astype(np.float32) / G.F255
    nz = c.X > 0
    assert (back[nz] != c.Xoff[nz]).mean() > 0.9 and np.array_equal(np.rint(c.X * G.F255).astype(np.float32) / G.F255, c.X)
