"""Shared pieces of the projection-mask search tests (tests/test_mask_search_cpu.py, tests/test_mask_search_gpu.py,
tests/test_gram_segments_gpu.py): the real XY fixture cut into three uneven "projections", the NumPy float64 twin of the mask
hooks, and scikit-learn's own GridSearchCV run live, once per mask, on the column subset."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_search_common as G  # noqa: E402
sys.path.pop(0)

# 682 columns as 264 + 372 + 46: the proportions of 3 872 : 5 457 : 682, none a multiple of 32
SEGMENTS = (264, 372, 46)
SUB_GRID = [{"C": [1, 10], "kernel": ["linear"]}, {"C": [1, 10], "gamma": [0.01, 0.1], "kernel": ["rbf"]}]
SCORE_KEYS = ["split%d_test_score" % k for k in range(5)] + ["mean_test_score", "std_test_score"]


def all_masks():
    from radar_ml_amd import ProjMask
    return [ProjMask(bool(b & 1), bool(b & 2), bool(b & 4)) for b in range(1, 8)]


def mask_bits(mask):
    return sum(1 << i for i in range(3) if mask[i])


def cols_of(mask, segments=SEGMENTS):
    start = np.concatenate([[0], np.cumsum(segments)])
    return np.concatenate([np.arange(start[i], start[i + 1]) for i in range(3) if mask[i]])


def segment_products(X, segments):
    """float64 inner products and squared norms per segment"""
    X64 = np.asarray(X, dtype=np.float64)
    start = np.concatenate([[0], np.cumsum(segments)])
    parts = [X64[:, start[s]:start[s + 1]] for s in range(len(segments))]
    return [p @ p.T for p in parts], [(p * p).sum(1) for p in parts]


def compose(Gs, ns, keys):
    """rml_gram_compose's expressions in NumPy: sums over the set bits in ascending s, d2 = (n_i + n_j) - 2 g"""
    out = []
    for bits, kind, gamma in keys:
        sel = [s for s in range(len(Gs)) if bits >> s & 1]
        g, n = Gs[sel[0]].copy(), ns[sel[0]].copy()
        for s in sel[1:]:
            g, n = g + Gs[s], n + ns[s]
        out.append(g if kind == "linear" else np.exp(-gamma * ((n[:, None] + n[None, :]) - 2.0 * g)))
    return out


def numpy_gram_masks(X, segments, keys, device=None):
    """float64 NumPy twin of radar_ml_amd.train._gram_masks (test oracle only)"""
    Gs, ns = segment_products(X, segments)
    return compose(Gs, ns, keys)


def subset_oracle(X, cols, kind, gamma):
    """the kernel matrix of the column subset, float64, the association of a plain Gram pass"""
    return G.numpy_gram(np.ascontiguousarray(np.asarray(X)[:, cols]), [(kind, gamma)])[0]


@functools.lru_cache(maxsize=None)
def live_searches(which):
    """GridSearchCV(SVC) live on X[:, cols] for each of the seven masks (``which``: 'sub' or 'full' grid); shared, never changed"""
    X, y = G.real_xy()
    grid = SUB_GRID if which == "sub" else G.GRID
    return tuple(G.sklearn_search(np.ascontiguousarray(X[:, cols_of(m)]), y, grid=grid) for m in all_masks())


def check_scores(ours, which, masks=None):
    """every mask's slice of cv_results_ equals the live search on the column subset, bit for bit; returns the live winner
    (first best over the masks in order)"""
    live = live_searches(which)
    every = all_masks()
    masks = every if masks is None else masks
    per = len(live[0].cv_results_["params"])
    assert len(ours.cv_results_["params"]) == per * len(masks)
    best = None
    for mi, m in enumerate(masks):
        ref = live[every.index(m)]
        sl = slice(mi * per, (mi + 1) * per)
        for key in SCORE_KEYS:
            assert np.array_equal(ours.cv_results_[key][sl], ref.cv_results_[key]), (m, key)
        for p, q in zip(ours.cv_results_["params"][sl], ref.cv_results_["params"]):
            assert p["proj_mask"] == m and {k: v for k, v in p.items() if k != "proj_mask"} == q
        assert list(ours.cv_results_["param_proj_mask"][sl]) == [m] * per
        if best is None or ref.best_score_ > best[1].best_score_:
            best = (m, ref, mi * per + ref.best_index_)
    assert ours.best_proj_mask_ == best[0]
    assert ours.best_params_ == best[1].best_params_ and "proj_mask" not in ours.best_params_
    assert ours.best_score_ == best[1].best_score_
    assert ours.best_index_ == best[2]
    assert ours.cv_results_["rank_test_score"][ours.best_index_] == 1
    assert ours.n_splits_ == 5
    return best[0], best[1]
