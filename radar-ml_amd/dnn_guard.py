"""The margin guard of the CNN row (dnn.py ``Classifier._guard``): float64 labels from a bf16 chain.

Rows of a probability table whose top-2 gap is too small for a bf16 chain are replaced by what exact-input arithmetic gives.  The
POLICY (:class:`MarginGuard`: which rows, how often, through which precision) is plain Python on tensors of any device; the DEVICE
OPERATIONS it needs -- the gaps, the candidate pick, one round's bookkeeping -- sit behind :class:`GuardOps`, whose CUDA form
(:class:`CudaOps`) is two kernels of csrc/guard.hip.

``last_guard`` (``MarginGuard.last``, ``Classifier.last_guard``) after a call -- the one list of its keys:
  rows               rows of the table
  rescored           rows re-scored in "x3" (every candidate of every round)
  rescored_x6        ... of those, rows whose x3 gap was below LABEL_GUARD_X3: re-scored in "x6"
  rescored_float64   ... of those, rows re-scored in float64 (x6 gap below LABEL_GUARD_X6, closest ties first)
  observed_error     largest |chain - x3| on the re-scored rows: the bf16 chain's error as this call saw it
  observed_error_x3  largest |x3 - x6| on the x6 rows
  observed_error_x6  largest |x6 - float64| on the float64 rows
  gap                the top-2 gap the call covered: every row below it was re-scored
  rounds             candidate sets re-scored (0: no row was below the gap)
  covered            False when the loop gave up (MAX_ROUNDS) before the gap covered four times the error seen
A call that has nothing to guard (no gap given, no rows, fewer than two classes) leaves rows, rescored, rescored_float64, rounds and
covered only.
"""
from collections import namedtuple

import numpy as np

# Rows whose top-2 probability gap is below this are re-scored.  The bf16 chain moves a probability by <= 3.4e-3 on trained weights
# (larger logits) and <= 4.8e-4 on random-init ones (measured against the float64 restatement, tests/test_nn_gpu.py
# DNN_BF16_PROBA_TOL / _RANDOM_INIT_TOL), i.e. a gap by <= 6.8e-3: 3 x that.
LABEL_GUARD = 2e-2
# Second level: the float32-class trunk (csrc/dnn_x3.hip, bf16 operand pairs) + float32 dense layers on exact inputs; rows whose gap
# there is below this go on.  Measured |x3 - float64|: 7.0e-6 on the trained bench model's candidate rows, 5e-7 at random init
# (tools/guard_profile.py; tests/test_nn_gpu.py::test_x3_trunk_is_float32_class asserts 4 x its own worst under this): 7 x that.
LABEL_GUARD_X3 = 5e-5
# Third level: the same kernel with three bf16 parts per operand ("x6": float32-class in the strict sense; measured 9.6e-7 / 1.1e-7
# on the same rows) on the rows whose x3 gap is below LABEL_GUARD_X3; rows whose gap there is below this go to float64.
LABEL_GUARD_X6 = 1e-5
LABEL_GUARD_F32 = LABEL_GUARD_X3        # (the name of rounds 1-5, when this stage ran PyTorch's float32 layers)

# The cascade a candidate set runs down, in order; behind the last stage comes the float64 tail.  ``marks_gap``: the stage's apply
# sets the rows' entries of the gap array to +inf (re-scored: never a candidate again) -- the first stage alone, the later ones
# see subsets of its rows.  ``count`` / ``error``: the last_guard keys the stage adds its rows / its largest change to.
Stage = namedtuple("Stage", "precision close marks_gap count error")
STAGES = (Stage("x3", LABEL_GUARD_X3, True, "rescored", "observed_error"),
          Stage("x6", LABEL_GUARD_X6, False, "rescored_x6", "observed_error_x3"))
MAX_ROUNDS = 4
FLOAT64_CHUNK = 32
HOST_PICK_ROWS = 4096


def weights_key(params):
    """What changes when one of ``params`` is written (optimizer step, load_state_dict, .to()): version counter and storage of each."""
    return tuple((p._version, p.data_ptr()) for p in params)


def top2_gaps(p):
    """top-2 gap per row; a row with a non-finite probability counts as a tie"""
    import torch
    top2 = torch.nan_to_num(p.float(), nan=0.0, posinf=0.0, neginf=0.0).topk(2, dim=1).values
    g = top2[:, 0] - top2[:, 1]
    return torch.where(torch.isfinite(p.float()).all(dim=1), g, torch.zeros_like(g))


def run_padded(fn, idx, size):
    """fn(rows) in launches of EXACTLY ``size`` rows (a short one padded by repeating its first row): every launch of a size has
    the same shape whatever the count"""
    import torch
    outs = []
    for s in range(0, int(idx.numel()), size):
        sel = idx[s:s + size]
        k = int(sel.numel())
        if k < size:
            sel = torch.cat([sel, sel[:1].expand(size - k)])
        outs.append(fn(sel)[:k])
    return torch.cat(outs)


class GuardOps:
    """What the policy asks of the device.  ``gaps(proba)`` -> (N,) float32 top-2 gaps, 0 for a row with a non-finite value;
    ``apply(proba, rows, fresh, thr_close, gap)``: proba[rows] <- fresh, gap[rows] <- +inf when ``gap`` is given; returns (largest
    |old - new| over the rows where both are finite, rows whose NEW gap is below thr_close, that test per row as a uint8 mask)."""

    def candidates(self, gap, thr):
        """The rows whose gap is below ``thr`` as an ascending int64 index tensor on the gaps' device; None when there are none."""
        import torch
        if int(gap.shape[0]) <= HOST_PICK_ROWS:
            # a few rows (dnn.py:373-381 predicts ONE target per call): the gaps cross to the host in one copy and the
            # candidates are picked there -- compare + nonzero on the device are three launches and a synchronisation
            idx = np.flatnonzero(gap.cpu().numpy() < thr)
            return torch.from_numpy(idx).to(gap.device) if idx.size else None
        cand = (gap < thr).nonzero().squeeze(1)                             # device -> host: the candidate count
        return cand if int(cand.numel()) else None


class CudaOps(GuardOps):
    """csrc/guard.hip: rml_dnn_top2_gap, and rml_dnn_guard_apply -- rows replaced, the largest change on them, the rows still near a
    tie, gap[rows] = inf in ONE launch, read back as one (error bits, count) pair."""

    def gaps(self, proba):
        import torch
        from . import _lib
        if not (proba.is_cuda and proba.dtype == torch.float32 and proba.stride(1) == 1 and proba.shape[1] <= 16):
            raise ValueError("_guard: a CUDA float32 (N, C <= 16) probability tensor expected")
        self.lib, self.dev, self.stats = _lib.load(), proba.device, None
        with torch.cuda.device(self.dev):
            self.ctx, self.stream = _lib.context(self.dev), _lib.stream_ptr(self.dev)
            g = torch.empty((int(proba.shape[0]),), dtype=torch.float32, device=self.dev)
            _lib.check(self.lib.rml_dnn_top2_gap(self.ctx, _lib.ptr(proba), int(proba.stride(0)), int(proba.shape[0]), int(proba.shape[1]),
                                                 _lib.ptr(g), self.stream), "rml_dnn_top2_gap")
        return g

    def candidates(self, gap, thr):
        import torch
        cand = GuardOps.candidates(self, gap, thr)
        if cand is not None and self.stats is None:
            self.stats = torch.zeros((2,), dtype=torch.int32, device=self.dev)   # shared by every apply of the call
        return cand

    def apply(self, proba, rows, fresh, thr_close, gap):
        import torch
        from . import _lib
        n = int(rows.numel())
        with torch.cuda.device(self.dev):
            close = torch.empty((n,), dtype=torch.uint8, device=self.dev)
            self.stats.zero_()
            _lib.check(self.lib.rml_dnn_guard_apply(self.ctx, _lib.ptr(proba), int(proba.stride(0)), int(proba.shape[1]), _lib.ptr(rows), n,
                                                    _lib.ptr(fresh), float(thr_close), _lib.ptr(gap), _lib.ptr(self.stats), _lib.ptr(close),
                                                    self.stream), "rml_dnn_guard_apply")
            sh = self.stats.cpu()                                           # device -> host: the error seen, the rows that go on
        return float(sh[:1].view(torch.float32)[0]), int(sh[1]), close


class MarginGuard:
    """The policy.  A round's candidates are the rows below the gap; ALL of them go down the cascade in one pass -- STAGES, then the
    float64 tail -- each stage on the rows the one before left near a tie.  The gap calibrates itself: the first stage measures the
    bf16 chain's error; if four times that error (a gap moves by at most twice a probability's error, twice again for margin)
    reaches past the gap covered so far, the rows in between are the next round.  The bound is EMPIRICAL: a row outside the covered
    gap whose bf16 error exceeds twice the largest error seen on the re-scored rows keeps its bf16 label.  The gap a call ends with
    is where the next call on the same weights starts (the same rows, the same bits when the call is repeated; one round instead
    of two in the steady state)."""

    def __init__(self):
        self.last = None
        self._key, self._gap = None, 0.0

    def run(self, proba, eps, rescore, ops, params):
        """Guard ``proba`` (N, C) in place and return it.  ``rescore(rows, precision)`` -> (len(rows), C) probabilities of those rows
        from exact inputs; ``ops``: a :class:`GuardOps`; ``params``: the weights the remembered gap belongs to."""
        rep = self.last = {"rows": int(proba.shape[0]), "rescored": 0, "rescored_float64": 0, "rounds": 0, "covered": True}
        if not eps or proba.shape[0] == 0 or proba.shape[1] < 2:
            return proba
        gap = ops.gaps(proba)
        rep.update(rescored_x6=0, observed_error=0.0, observed_error_x3=0.0, observed_error_x6=0.0)
        key, thr = weights_key(params), float(eps)
        if self._key == key:
            thr = max(thr, self._gap)
        while True:
            cand = ops.candidates(gap, thr)
            if cand is not None:
                rep["rounds"] += 1
                self._cascade(proba, cand, rescore, ops, gap, rep)
            err = rep["observed_error"]
            if thr >= min(4.0 * err, 1.0):
                break
            if rep["rounds"] >= MAX_ROUNDS:
                rep["covered"] = False
                break
            thr = min(8.0 * err, 1.0)
        rep["gap"] = thr
        if rep["rounds"]:
            self._key, self._gap = key, thr
        return proba

    def _cascade(self, proba, rows, rescore, ops, gap, rep):
        for st in STAGES:
            fresh = rescore(rows, st.precision).float().contiguous()
            err, still, close = ops.apply(proba, rows, fresh, st.close, gap if st.marks_gap else None)
            rep[st.count] += int(rows.numel())
            rep[st.error] = max(rep[st.error], err)
            if not still:
                return
            sel = close.nonzero().squeeze(1)
            rows = rows[sel]
        self._float64_tail(proba, rows, fresh[sel], rescore, rep)

    @staticmethod
    def _float64_tail(proba, rows, p6, rescore, rep):
        """Last stage: ``rows`` (their x6 probabilities ``p6`` have a top-2 gap below LABEL_GUARD_X6), closest ties first,
        FLOAT64_CHUNK at a time through ``rescore(rows, "float64")``; the pass stops at the first chunk boundary whose gap is at
        least eight times the largest |x6 - float64| seen (at least 1e-6)."""
        import torch
        g6 = top2_gaps(p6)
        order = torch.argsort(g6)
        gs = g6[order].cpu()                                                # ascending, on the host
        rows, p6 = rows[order], p6[order]
        n, pos, e6 = int(rows.numel()), 0, 0.0
        while pos < n:
            idx = rows[pos:pos + FLOAT64_CHUNK]
            p64 = run_padded(lambda r: rescore(r, "float64"), idx, FLOAT64_CHUNK)
            e6 = max(e6, float((p6[pos:pos + FLOAT64_CHUNK].double() - p64.double()).abs().max()))
            proba[idx] = p64.to(proba.dtype)
            pos += int(idx.numel())
            if pos < n and float(gs[pos]) >= max(8.0 * e6, 1e-6):
                break
        rep["rescored_float64"] += pos
        rep["observed_error_x6"] = max(rep["observed_error_x6"], e6)
