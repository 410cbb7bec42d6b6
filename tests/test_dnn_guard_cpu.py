"""The CNN row's margin guard without a GPU: the policy of radar-ml_amd/dnn_guard.py decision by decision, by value, on a stand-in for
the device operations (tests/dnn_guard_common.py); the weight-pack cache, the route choice of rescore_exact and
rml_dnn_trunk_kblock_supported (host code) of radar-ml_amd/dnn.py.

Every table below is made of dyadic numbers -- 0.5 +- k * 2^-24 -- so each gap, error and threshold product is exact in float32 and
in Python's floats, and the expected values are written down, not computed by the code under test."""
import importlib

import numpy as np
import pytest
import torch

from dnn_guard_common import host_ops

U = 2.0 ** -24          # probabilities are 0.5 +- k * U: exact in float32
OFF = {"rescored": 0, "rescored_float64": 0, "rounds": 0, "covered": True}
ZERO = dict(OFF, rescored_x6=0, observed_error=0.0, observed_error_x3=0.0, observed_error_x6=0.0)


@pytest.fixture(scope="module")
def G(rml):
    return importlib.import_module("radar_ml_amd.dnn_guard")


def table(halfgaps, dtype=torch.float32):
    """rows [0.5 + a, 0.5 - a, 0]: top-2 gap 2 * a"""
    a = torch.as_tensor(halfgaps, dtype=torch.float64)
    return torch.stack([0.5 + a, 0.5 - a, torch.zeros_like(a)], dim=1).to(dtype)


class Rescore:
    """rescore(rows, precision) from fixed tables; writes down every call"""

    def __init__(self, **tables):
        self.tables, self.calls = tables, []

    def __call__(self, rows, precision):
        self.calls.append((precision, rows.tolist()))
        return self.tables[precision][rows]


def run(G, proba, eps, rescore, guard=None, params=()):
    guard, ops = guard or G.MarginGuard(), host_ops()
    out = guard.run(proba, eps, rescore, ops, params)
    assert out is proba
    return guard, ops


@pytest.mark.parametrize("eps,shape", [(None, (5, 3)), (0, (5, 3)), (2e-2, (0, 3)), (2e-2, (5, 1))])
def test_nothing_to_guard(G, eps, shape):
    proba = torch.full(shape, 0.5)
    keep = proba.clone()
    guard, ops = run(G, proba, eps, Rescore())
    assert torch.equal(proba, keep) and ops.calls == []
    assert guard.last == dict(OFF, rows=shape[0])


def test_no_row_below_the_gap(G):
    eps = 2.0 ** -6
    proba = table([2.0 ** -7, 0.25, 2.0 ** -4])                 # gaps 2^-6 (not below), 0.5, 2^-3
    keep = proba.clone()
    rs = Rescore()
    lin = torch.nn.Linear(2, 2)
    guard, ops = run(G, proba, eps, rs, params=list(lin.parameters()))
    assert rs.calls == [] and torch.equal(proba, keep)
    assert ops.calls == [("gaps",), ("candidates", eps, [])]
    assert guard.last == dict(ZERO, rows=3, gap=eps, rounds=0)
    # nothing remembered: the next call on the same weights starts at ITS eps, not at this one
    run(G, proba, 2.0 ** -9, rs, guard, list(lin.parameters()))
    assert guard.last["gap"] == 2.0 ** -9


def test_one_round(G):
    eps = 2.0 ** -6
    a = [0.25, 2.0 ** -9, 0.125, 2.0 ** -8, 0.0, 2.0 ** -7]      # gaps below eps = 2^-6: rows 1, 3, 4 (row 5 sits ON it)
    b = [0.0, 2.0 ** -9 + 2.0 ** -10, 0.0, 2.0 ** -8 - 2.0 ** -9, 2.0 ** -10, 0.0]
    proba, x3 = table(a), table(b)
    rs = Rescore(x3=x3)
    guard, ops = run(G, proba, eps, rs)
    assert rs.calls == [("x3", [1, 3, 4])]
    want = table(a)
    want[[1, 3, 4]] = x3[[1, 3, 4]]
    assert torch.equal(proba, want)
    # errors |a - b|: 2^-10, 2^-9, 2^-10; four times the largest is 2^-7 <= eps: covered in one round
    assert guard.last == dict(ZERO, rows=6, rescored=3, observed_error=2.0 ** -9, gap=eps, rounds=1)
    assert ops.calls == [("gaps",), ("candidates", eps, [1, 3, 4]), ("apply", [1, 3, 4], G.LABEL_GUARD_X3, True)]


WIDEN_A = [2.0 ** -8, 0.25, 2.0 ** -7, 2.0 ** -6, 2.0 ** -5, 2.0 ** -9, 3 * 2.0 ** -7]   # gaps 2^-7, .5, 2^-6, 2^-5, 2^-4, 2^-8, 3 * 2^-6
WIDEN_B = [2.0 ** -8 + 2.0 ** -7, 0.0, 2.0 ** -7 + 2.0 ** -9, 2.0 ** -6 + 2.0 ** -8, 0.0, 2.0 ** -9, 3 * 2.0 ** -7 - 2.0 ** -8]


def test_widening(G):
    """eps = 2^-6; round 1: rows 0 and 5 (gaps 2^-7, 2^-8), error 2^-7 on row 0 -> 4 * err = 2^-5 > eps: the gap becomes 8 * err = 2^-4;
    round 2: rows 2 (gap == eps), 3, 6 -- not row 4 (gap == 2^-4, not below), not rows 0 and 5 again (row 5's x3 gap is still 2^-8)"""
    eps = 2.0 ** -6
    proba, x3 = table(WIDEN_A), table(WIDEN_B)
    rs = Rescore(x3=x3)
    guard, ops = run(G, proba, eps, rs)
    assert rs.calls == [("x3", [0, 5]), ("x3", [2, 3, 6])]
    want = table(WIDEN_A)
    want[[0, 5, 2, 3, 6]] = x3[[0, 5, 2, 3, 6]]
    assert torch.equal(proba, want)
    assert guard.last == dict(ZERO, rows=7, rescored=5, observed_error=2.0 ** -7, gap=2.0 ** -4, rounds=2)
    assert [c for c in ops.calls if c[0] == "candidates"] == [("candidates", eps, [0, 5]), ("candidates", 2.0 ** -4, [2, 3, 6])]


def test_remembered_gap(G):
    """the gap a call ended with is where the next call on the same weights starts; a write to any parameter forgets it"""
    eps = 2.0 ** -6
    lin = torch.nn.Linear(2, 2)
    params = list(lin.parameters())
    guard, _ = run(G, table(WIDEN_A), eps, Rescore(x3=table(WIDEN_B)), params=params)
    assert guard.last["rounds"] == 2 and guard.last["gap"] == 2.0 ** -4
    rs = Rescore(x3=table(WIDEN_B))
    run(G, table(WIDEN_A), eps, rs, guard, params)
    assert rs.calls == [("x3", [0, 2, 3, 5, 6])]                 # one round, at 2^-4 from the start
    assert guard.last == dict(ZERO, rows=7, rescored=5, observed_error=2.0 ** -7, gap=2.0 ** -4, rounds=1)
    with torch.no_grad():
        lin.bias.add_(1.0)
    rs = Rescore(x3=table(WIDEN_B))
    run(G, table(WIDEN_A), eps, rs, guard, params)
    assert rs.calls == [("x3", [0, 5]), ("x3", [2, 3, 6])] and guard.last["rounds"] == 2


def test_an_error_that_grows_every_round_gives_up(G):
    """round k's rows show an error whose fourfold lies beyond the gap just covered: eps = 2^-10 -> 2^-7 -> 2^-4 -> 2^-1, then the
    fourth round's error 2^-2 asks for 1 > 2^-1: not covered"""
    a = [2.0 ** -12, 2.0 ** -9, 2.0 ** -6, 2.0 ** -3, 0.375]     # gaps 2^-11, 2^-8, 2^-5, 2^-2, 0.75
    b = [2.0 ** -12 + 2.0 ** -10, 2.0 ** -9 + 2.0 ** -7, 2.0 ** -6 + 2.0 ** -4, 2.0 ** -3 - 2.0 ** -2, 0.0]
    proba, x3 = table(a), table(b)
    rs = Rescore(x3=x3)
    guard, ops = run(G, proba, 2.0 ** -10, rs)
    assert rs.calls == [("x3", [0]), ("x3", [1]), ("x3", [2]), ("x3", [3])]
    want = table(a)
    want[:4] = x3[:4]
    assert torch.equal(proba, want)
    assert guard.last == dict(ZERO, rows=5, rescored=4, observed_error=2.0 ** -2, gap=2.0 ** -1, rounds=4, covered=False)
    assert guard.last["covered"] is False


def cascade_tables(n64, seed):
    """100 rows, all candidates (chain gap 2^-8).  x3 leaves rows 0..9 clear (gap 2^-13 >= LABEL_GUARD_X3) and the other 90 near a tie
    (2^-15); x6 leaves 7 of those clear (2^-16 >= LABEL_GUARD_X6) and gives ``n64`` rows the gaps 1..n64 units of 2^-23 (all below
    LABEL_GUARD_X6 = 1e-5 = 83.9 units) in a shuffled order; float64 differs from x6 by 2^-20 on the row with the smallest gap and by
    2^-22 elsewhere."""
    assert 90 - n64 == 7
    rng = np.random.default_rng(seed)
    a3 = np.full(100, 2.0 ** -16)
    a3[:10] = 2.0 ** -14
    units = np.zeros(100)
    near = rng.permutation(np.arange(10, 100))
    units[near[:n64]] = np.arange(1, n64 + 1)
    a6 = units * U
    a6[near[n64:]] = 2.0 ** -17
    a6[:10] = a3[:10]                                            # (never asked for)
    e = np.full(100, 2.0 ** -22)
    e[near[0]] = 2.0 ** -20
    order64 = near[:n64].tolist()                                # ascending x6 gap
    return table(np.full(100, 2.0 ** -9)), table(a3), table(a6), table(a6 + e, torch.float64), sorted(near.tolist()), sorted(near[:n64].tolist()), order64


def test_cascade_stops_float64_at_a_chunk_boundary(G):
    """83 rows reach float64 with x6 gaps 1..83 units; the largest |x6 - float64| is 2^-20 (first chunk), so the pass stops at the first
    chunk boundary whose gap is >= 8 * 2^-20 = 64 units: behind the second chunk (the 65th gap is 65 units), 64 rows re-scored"""
    proba, x3, x6, f64, rows6, rows64, order64 = cascade_tables(83, 1)
    rs = Rescore(x3=x3, x6=x6, float64=f64)
    guard, ops = run(G, proba, 2.0 ** -6, rs)
    assert rs.calls == [("x3", list(range(100))), ("x6", rows6), ("float64", order64[:32]), ("float64", order64[32:64])]
    assert ops.calls == [("gaps",), ("candidates", 2.0 ** -6, list(range(100))), ("apply", list(range(100)), G.LABEL_GUARD_X3, True),
                         ("apply", rows6, G.LABEL_GUARD_X6, False)]                  # the x6 apply: no gap array
    want = x3.clone()
    want[rows6] = x6[rows6]
    want[order64[:64]] = f64[order64[:64]].float()
    assert torch.equal(proba, want)
    # |chain - x3| = 2^-9 - 2^-16 on the near rows; |x3 - x6| = 2^-16 - 1 unit on the row with the smallest x6 gap
    assert guard.last == {"rows": 100, "rescored": 100, "rescored_x6": 90, "rescored_float64": 64, "observed_error": 2.0 ** -9 - 2.0 ** -16,
                          "observed_error_x3": 2.0 ** -16 - U, "observed_error_x6": 2.0 ** -20, "gap": 2.0 ** -6, "rounds": 1, "covered": True}
    assert set(rows64) >= set(order64[:64])


def test_cascade_pads_a_short_float64_chunk(G):
    """40 rows reach float64, all below the stopping gap: 32 rows, then 8 rows padded to 32 by repeating the chunk's first row"""
    rng = np.random.default_rng(2)
    near = rng.permutation(100)[:40]
    a6 = np.full(100, 2.0 ** -17)
    a6[near] = np.arange(1, 41) * U
    proba, x3, x6 = table(np.full(100, 2.0 ** -9)), table(np.full(100, 2.0 ** -16)), table(a6)
    e = np.full(100, 2.0 ** -22)
    e[near[0]] = 2.0 ** -20
    f64 = table(a6 + e, torch.float64)
    rs = Rescore(x3=x3, x6=x6, float64=f64)
    guard, _ = run(G, proba, 2.0 ** -6, rs)
    order = near.tolist()
    assert rs.calls == [("x3", list(range(100))), ("x6", list(range(100))), ("float64", order[:32]), ("float64", order[32:] + [order[32]] * 24)]
    want = x6.clone()
    want[order] = f64[order].float()
    assert torch.equal(proba, want)
    assert guard.last == {"rows": 100, "rescored": 100, "rescored_x6": 100, "rescored_float64": 40, "observed_error": 2.0 ** -9 - 2.0 ** -16,
                          "observed_error_x3": 2.0 ** -16 - U, "observed_error_x6": 2.0 ** -20, "gap": 2.0 ** -6, "rounds": 1, "covered": True}


def test_non_finite_rows_are_candidates_and_say_nothing_about_the_error(G):
    proba = table([0.25, 0.25, 0.25, 2.0 ** -9])
    proba[0, 1] = float("nan")
    proba[1, 0] = float("inf")
    proba[2, 2] = float("-inf")
    x3 = table([0.125, 0.125, 0.125, 2.0 ** -9 + 2.0 ** -12])
    rs = Rescore(x3=x3)
    guard, ops = run(G, proba, 2.0 ** -6, rs)
    assert rs.calls == [("x3", [0, 1, 2, 3])]                    # gap 0 for the three non-finite rows
    assert torch.equal(proba, x3)
    assert guard.last == dict(ZERO, rows=4, rescored=4, observed_error=2.0 ** -12, gap=2.0 ** -6, rounds=1)
    # alone, they leave the error at zero
    proba = table([0.25, 0.25])
    proba[0, 0] = float("nan")
    guard, _ = run(G, proba, 2.0 ** -6, Rescore(x3=table([0.125, 0.125])))
    assert guard.last == dict(ZERO, rows=2, rescored=1, gap=2.0 ** -6, rounds=1)


def test_host_pick_and_device_pick_choose_the_same_rows(G):
    """N = 4096 picks on the host (NumPy), N = 4097 with tensor operations: the same rows on the same gaps, at values around the
    threshold's float32 neighbours too"""
    rng = np.random.default_rng(3)
    thr = 2e-2
    g = rng.uniform(0, 0.05, 4097).astype(np.float32)
    t32 = np.float32(thr)
    g[:6] = [t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1)), 0.0, np.inf, thr / 2]
    g[4096] = 1.0                                                # the extra row is no candidate
    g = torch.from_numpy(g)
    ops = G.GuardOps()
    host, device = ops.candidates(g[:4096], thr), ops.candidates(g, thr)
    assert host.dtype == device.dtype == torch.int64 and torch.equal(host, device)
    want = np.flatnonzero(g.numpy().astype(np.float64) < float(t32))      # below the threshold as float32 holds it
    assert host.tolist() == want.tolist() and 0 not in want and 1 in want and 2 not in want
    assert ops.candidates(torch.ones(4096), thr) is None and ops.candidates(torch.ones(4097), thr) is None


# ---- radar-ml_amd/dnn.py: the weight-pack cache -----------------------------------------------------------------
def _flat(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, dict):
        v = list(v.values())
    return [t for x in v if x is not None and not isinstance(x, int) for t in _flat(x)]


def test_weight_packs_are_rebuilt_when_their_parameters_are_written(rml):
    dnn = importlib.import_module("radar_ml_amd.dnn")
    torch.manual_seed(0)
    m = dnn.Classifier([(8, 16, 1)] * 3, 3)

    def packs():
        return {"conv": m._conv_packs(), "dense": m._dense_packs(), "exact": m._exact_weights(torch.float32)}
    p0 = packs()
    p1 = packs()
    assert all(p1[k] is p0[k] for k in p0) and m._tail_weights() is p0["dense"]["bf16"] and m._tail_f32 is p0["dense"]["f32"]
    # contents: one conv pack, w2's dtype alone differs; the tail operands of csrc/dense.hip
    w1, b1, w2, b2 = p0["conv"]["x3"]
    assert w1.shape == (3, 64, 9) and b1.shape == (3, 64) and w2.shape == (3, 32, 576) and b2.shape == (3, 32) and w2.dtype == torch.float32
    assert torch.equal(w2[1], m.branches[1][1].conv.weight.detach().permute(0, 2, 3, 1).reshape(32, 576))
    bf = p0["conv"]["bf16"]
    assert bf[0] is w1 and bf[1] is b1 and bf[3] is b2 and bf[2].dtype == torch.bfloat16 and torch.equal(bf[2], w2.to(torch.bfloat16))
    assert torch.equal(m._tail_f32[1], m.fc2.weight.detach().t()) and m._tail_f32[1].is_contiguous()
    with torch.no_grad():
        m.branches[2][0].conv.bias.add_(1.0)                     # one conv parameter: the conv packs (and the all-parameter copies)
    p2 = packs()
    assert p2["conv"] is not p0["conv"] and p2["dense"] is p0["dense"] and p2["exact"] is not p0["exact"]
    assert torch.equal(p2["conv"]["x3"][1][2], m.branches[2][0].conv.bias.detach())
    with torch.no_grad():
        m.fc3.weight.mul_(2.0)                                   # one dense parameter: the dense packs
    p3 = packs()
    assert p3["conv"] is p2["conv"] and p3["dense"] is not p2["dense"] and p3["exact"] is not p2["exact"]
    assert torch.equal(m._tail_f32[3], m.fc3.weight.detach())
    m.to(torch.float64)                                          # new storage under every parameter: all of them
    p4 = packs()
    assert all(p4[k] is not p3[k] for k in p3)
    old = {t.data_ptr() for k in p3 for t in _flat(p3[k])}
    assert not old & {t.data_ptr() for k in p4 for t in _flat(p4[k])}


def _parent_route(rows, N, fused_possible, host):
    """the if / elif ladder rescore_exact had before it was split into routes"""
    fused = fused_possible and not host
    if fused and rows is not None and 2 * rows < N:
        return "fused_gather"
    elif rows is None:
        return "all"
    elif 2 * rows >= N:
        return "dense_blocks"
    return "gather"


def test_rescore_route_choice(rml):
    dnn = importlib.import_module("radar_ml_amd.dnn")
    seen = set()
    for N in (1, 2, 7, 300):
        for rows in (None, 0, 1, N // 2 - 1, N // 2, (N + 1) // 2, N // 2 + 1, N, 2 * N):
            if rows is not None and rows < 0:
                continue
            for fused in (False, True):
                for host in (False, True):
                    got = dnn.rescore_route(rows, N, fused, host)
                    assert got == _parent_route(rows, N, fused, host), (rows, N, fused, host)
                    seen.add(got)
    assert seen == {"fused_gather", "all", "dense_blocks", "gather"}
    assert dnn.rescore_route(150, 300, True, False) == "dense_blocks" and dnn.rescore_route(149, 300, True, False) == "fused_gather"
    assert dnn.rescore_route(149, 300, True, True) == "gather" and dnn.rescore_route(149, 300, False, False) == "gather"


def test_kblock_supported_asks_the_kernels_layout(rml):
    """rml_dnn_trunk_kblock_supported (host code of csrc/dnn.hip, answered from RfLayout) against the arithmetic
    Classifier.kblock_supported restated until now"""
    from radar_ml_amd import _lib
    lib = _lib.load()

    def restated(H, W):
        rf_lds = 8 * (((H + 4) * (W + 4) * 2 + 15) // 16 * 16) + 36 * 1024 + 160
        return H % 4 == 0 and W % 8 == 0 and ((H // 4) * (W // 4)) % 2 == 0 and rf_lds <= 160 * 1024
    n_true = 0
    for H in range(4, 161, 4):
        for W in range(4, 161, 4):
            assert bool(lib.rml_dnn_trunk_kblock_supported(H, W)) == restated(H, W), (H, W)
            n_true += restated(H, W)
    assert 0 < n_true < 40 * 40
    assert lib.rml_dnn_trunk_kblock_supported(80, 80) == 1
    # 8 planes of (H + 4) x (W + 4) bf16 + 36 KB + 160 B within 160 KB: 88 x 80 is the last multiple of 8 rows that fits at W = 80
    assert lib.rml_dnn_trunk_kblock_supported(88, 80) == 1 and lib.rml_dnn_trunk_kblock_supported(96, 80) == 0
    assert lib.rml_dnn_trunk_kblock_supported(0, 80) == 0 and lib.rml_dnn_trunk_kblock_supported(80, -8) == 0
    dnn = importlib.import_module("radar_ml_amd.dnn")
    assert dnn.Classifier([(80, 80, 1)] * 3, 3).kblock_supported(80, 80)
    assert not dnn.Classifier([(80, 80, 1)] * 3, 17).kblock_supported(80, 80)            # the dense tail's class limit stays in Python
    assert not dnn.Classifier([(96, 80, 1)] * 3, 3).kblock_supported(96, 80)
