"""Shared by test_sgan_guard_cpu.py and test_sgan_guard_gpu.py: plane sets whose float64 labels hang on margins a bf16 chain cannot
resolve.  For a test model (sgan_infer_common.make_model) pairs of plane sets (xa, xb) with different float64 labels are taken and t
in x(t) = float32((1 - t) xa + t xb) is bisected, x(t) evaluated with the float64 CPU model (a .double() copy through
sgan_infer_common.plain_eval), until the float64 top-2 gap falls below a per-row target (and stays above a third of it); the targets are log-spaced
from 1e-2 down to 1e-6.  These rows are mixed with clearly decided ones.  Everything here comes from the float64 reference alone."""
import copy
import functools

import numpy as np

from sgan_infer_common import make_model, make_planes, plain_eval

GAP_FLOOR = 1e-9            # every row's float64 gap is at least this: summation order in float64 cannot decide a label
DECIDED = 0.2               # a decided row's float64 gap exceeds this
DECADES = ((1e-6, 1e-5), (1e-5, 1e-4), (1e-4, 1e-3), (1e-3, 1e-2))
# (H, W, classes, seed, near-tie rows, decided rows, planes drawn to pick pairs from)
SMALL = (16, 16, 3, 61, 12, 12, 48)
LARGE = (128, 128, 3, 62, 5, 3, 6)


def top2_gap(p):
    top2 = p.topk(2, dim=1).values
    return top2[:, 0] - top2[:, 1]


@functools.lru_cache(maxsize=None)
def fixture(H, W, C, seed, n_near, n_dec, pool):
    """(model on the CPU in float32, [xz, yz, xy] float32 (N, H, W), float64 probabilities (N, C), float64 gaps (N,), targets (N,):
    the gap a near-tie row was bisected under, 0 for a decided row).  Near-tie and decided rows alternate while both last."""
    import torch
    model = make_model(H, W, C, seed)
    ref = copy.deepcopy(model).double()
    xs = make_planes(pool, H, W, seed)
    p = plain_eval(ref, xs)[1]
    lab, gap = p.argmax(dim=1), top2_gap(p)
    decided = [i for i in range(pool) if float(gap[i]) > DECIDED]
    assert len(decided) >= n_dec + 1, "the planes drawn hold too few decided rows (%d)" % len(decided)
    # pairs (a, b): a decided row and the next row (cyclically) whose float64 label is another one
    pairs = []
    for k in range(n_near):
        a = decided[k % len(decided)]
        b = next(j for j in ((a + 1 + k // len(decided) + d) % pool for d in range(pool)) if int(lab[j]) != int(lab[a]))
        pairs.append((a, b))
    targets = np.logspace(-2, -6, n_near) if n_near > len(DECADES) + 1 else np.array([3e-3, 3e-4, 1e-4, 3e-5, 3e-6][:n_near])
    xa = [x[[a for a, _ in pairs]].double() for x in xs]
    xb = [x[[b for _, b in pairs]].double() for x in xs]
    la = lab[[a for a, _ in pairs]]
    lo, hi = torch.zeros(n_near, dtype=torch.float64), torch.ones(n_near, dtype=torch.float64)
    tgt = torch.from_numpy(targets)
    done = torch.zeros(n_near, dtype=torch.bool)
    near = [torch.zeros((n_near, H, W), dtype=torch.float32) for _ in range(3)]
    for _ in range(64):
        todo = (~done).nonzero().squeeze(1)
        if todo.numel() == 0:
            break
        mid = 0.5 * (lo[todo] + hi[todo])
        t = mid[:, None, None]
        xm = [((1.0 - t) * a[todo] + t * b[todo]).float() for a, b in zip(xa, xb)]
        pm = plain_eval(ref, xm)[1]
        # the signed margin of the first set's label: positive and decided at t = 0, negative at t = 1, continuous in between up to
        # the planes' float32 rounding.  A row is taken when it lands in [target / 3, target); where it is positive it IS the top-2 gap
        other = pm.clone()
        other[torch.arange(len(todo)), la[todo]] = -1.0
        margin = pm[torch.arange(len(todo)), la[todo]] - other.max(dim=1).values
        hit = (margin < tgt[todo]) & (margin >= tgt[todo] / 3.0)
        for src, dst in zip(xm, near):
            dst[todo[hit]] = src[hit]
        done[todo[hit]] = True
        above = margin >= tgt[todo]
        lo[todo] = torch.where(above, mid, lo[todo])
        hi[todo] = torch.where(above, hi[todo], mid)
    assert bool(done.all()), "the bisection did not reach every target gap"
    dec = [x[decided[:n_dec]] for x in xs]
    order, tlist, i, j = [], [], 0, 0
    while i < n_near or j < n_dec:
        if i < n_near:
            order.append(("n", i)); tlist.append(float(targets[i])); i += 1
        if j < n_dec:
            order.append(("d", j)); tlist.append(0.0); j += 1
    planes = [torch.stack([(nr if kind == "n" else dc)[k] for kind, k in order]) for nr, dc in zip(near, dec)]
    p64 = plain_eval(ref, planes)[1]
    return model, planes, p64, top2_gap(p64), torch.tensor(tlist, dtype=torch.float64)


def check_fixture(fx):
    """the conditions on a fixture, from the float64 reference alone"""
    _, planes, p64, gap, targets = fx
    n = int(p64.shape[0])
    assert p64.dtype.is_floating_point and p64.element_size() == 8 and all(x.shape[0] == n for x in planes)
    assert float(gap.min()) >= GAP_FLOOR, "a row's float64 gap is %.3e" % float(gap.min())
    for lo, hi in DECADES:
        assert int(((gap >= lo) & (gap < hi)).sum()) >= 1, "no row with a float64 gap in [%g, %g)" % (lo, hi)
    assert 3 * int((gap > DECIDED).sum()) >= n, "fewer than a third of the rows are decided"
    near = targets > 0
    assert bool((gap[near] < targets[near]).all()) and bool((gap[near] >= targets[near] / 3.0).all()) and bool((gap[~near] > DECIDED).all())
    return n
