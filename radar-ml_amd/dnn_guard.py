"""The margin guard of the CNN row (dnn.py ``Classifier._guard``) and of the SGAN classifier (sgan.py ``Discriminator._guard``, with its own
stage thresholds): float64 labels from a bf16 chain.

Rows of a probability table whose top-2 gap is too small for a bf16 chain are replaced by what exact-input arithmetic gives.  The
POLICY (:class:`MarginGuard`: which rows, how often, through which precision) is plain Python on tensors of any device; the DEVICE
OPERATIONS it needs -- the gaps, the candidate pick, one round's bookkeeping -- sit behind :class:`GuardOps`, whose CUDA form
(:class:`CudaOps`) is two kernels of csrc/guard.hip.  :class:`ExactRescore` holds the passes of ``rescore_exact`` -- volumes to exact planes to the
model's ``forward_exact`` -- that both models share.

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


def rescore_route(n_rows, N, fused, host):
    """Which pass of ``rescore_exact`` scores ``n_rows`` (None: all) of ``N`` frames.  ``fused``: precision, mode, planes
    and volumes fit rml_dnn_exact_features; ``host``: host volumes.  Sparse: fewer than half of the frames are wanted."""
    sparse = n_rows is not None and 2 * n_rows < N
    if sparse and fused and not host:
        return "fused_gather"       # one library call per pass: gather, projection, resize, trunk
    if n_rows is None:
        return "all"
    return "gather" if sparse else "dense_blocks"


class ExactRescore:
    """The passes of ``rescore_exact`` that do not depend on the model (dnn.py ``Classifier``, sgan.py ``Discriminator``): volumes ->
    exact projection (``common.process_volumes(scale=False)``) -> Pillow-bit-identical float32 planes
    (``nn_common.preprocess_features``) -> the model's ``forward_exact(xz, yz, xy, precision=...)``, in bounded passes, by the route
    :func:`rescore_route` picks.  The model brings ``forward_exact``, ``n_classes`` and ``parameters()``; one that can go from
    volumes to probabilities in one library call per pass says so in ``_one_call_route`` and does it in ``_one_call``."""

    # frames per pass of rescore_exact: the gathered volumes, their float rows, three float32 planes and the float32 features each
    RESCORE_BYTES = 2 << 30
    # frames per block of its dense route (nothing is gathered there: a pass is bounded by its intermediates -- 270 KB per frame
    # at the CNN's 80 x 80 -- not by RESCORE_BYTES of volumes)
    RESCORE_BLOCK = 16384

    def _one_call_route(self, volumes, rescale, mode, precision):
        return False

    def _one_call(self, volumes, rows, rescale, mode, precision):
        raise NotImplementedError

    def _rescore(self, volumes, rescale, mode, precision, rows, ijk):
        import torch
        from . import common, nn_common
        N = int(volumes.shape[0])
        dims = tuple(int(v) for v in volumes.shape[1:])
        step = max(64, min(16384, self.RESCORE_BYTES // max(1, dims[0] * dims[1] * dims[2] * volumes.element_size())))
        host = not volumes.is_cuda
        dev = next(self.parameters()).device
        if mode == "slice":
            return self._rescore_slices(volumes, rescale, precision, rows, ijk, step)

        def score(v, pick=None):
            if host:
                v = v.to(dev)
            feat = common.process_volumes(v, mode=mode, scale=False)
            if pick is not None:
                feat = feat[pick]
            xs = nn_common.preprocess_features(feat, dims, rescale, out_dtype="float32")
            return self.forward_exact(*xs, precision=precision)

        with torch.no_grad():
            fused = not host and bool(self._one_call_route(volumes, rescale, mode, precision))
            route = rescore_route(None if rows is None else int(rows.numel()), N, fused, host)
            if route == "dense_blocks":
                return self._rescore_dense_blocks(volumes, rows, score)
            if route == "fused_gather":
                outs = [self._one_call(volumes, rows[s:s + step], rescale, mode, precision) for s in range(0, int(rows.numel()), step)]
            elif route == "all":
                outs = [score(volumes[s:s + step]) for s in range(0, N, step)]
            else:
                outs = self._rescore_gather(volumes, rows, step, score)
        return torch.cat(outs) if len(outs) != 1 else outs[0]

    def _rescore_slices(self, volumes, rescale, precision, rows, ijk, step):
        """:meth:`_rescore` on target slices.  All rows: blocks of frames with their (T,3) indices, no volume duplicated; an index
        tensor: the frames of ``step`` rows gathered (a frame once per wanted target of it: the guard asks for a handful of rows)."""
        import torch
        from . import common, nn_common
        if ijk is None:
            raise ValueError("rescore_exact: mode='slice' needs ijk")
        N = int(volumes.shape[0])
        dims = tuple(int(v) for v in volumes.shape[1:])
        host = not volumes.is_cuda
        dev = next(self.parameters()).device
        ijk, T = nn_common.slice_targets_arg(ijk, N)
        ijk = ijk.reshape(N, T, 3)
        if rows is not None and 2 * int(rows.numel()) >= N * T:
            # at least half of the rows are wanted (a model without margins): every row by blocks of frames, no gather, and pick
            return self._rescore_slices(volumes, rescale, precision, None, ijk, step)[rows.to(dev)]

        def score(v, idx):
            feat = common.process_volumes(v.to(dev) if host else v, mode="slice", ijk=idx, scale=False)
            xs = nn_common.preprocess_features(feat, dims, rescale, out_dtype="float32")
            return self.forward_exact(*xs, precision=precision)

        with torch.no_grad():
            if rows is None:
                fstep = max(1, step // T)
                outs = [score(volumes[s:s + fstep], ijk[s:s + fstep]) for s in range(0, N, fstep)]
            else:
                flat = ijk.reshape(N * T, 3)
                outs = []
                for s in range(0, int(rows.numel()), step):
                    r = rows[s:s + step]
                    frames, _ = nn_common.slice_row_targets(r, T)
                    outs.append(score(volumes[frames.cpu() if host else frames.to(volumes.device)], flat[r.to(flat.device)]))
            if not outs:
                return torch.zeros((0, self.n_classes), dtype=torch.float64 if precision == "float64" else torch.float32, device=dev)
        return torch.cat(outs) if len(outs) != 1 else outs[0]

    @staticmethod
    def _rescore_gather(volumes, rows, step, score):
        """the sparse route for host volumes and for what the library call does not take: gather ``step`` frames, score them"""
        host = not volumes.is_cuda
        return [score(volumes[rows[s:s + step].cpu() if host else rows[s:s + step]]) for s in range(0, int(rows.numel()), step)]

    def _rescore_dense_blocks(self, volumes, rows, score):
        """the dense route: every block of RESCORE_BLOCK contiguous frames that holds a wanted frame is projected whole, the wanted
        feature rows picked (in ascending order) and their probabilities put back in the order of ``rows``"""
        import torch
        N, blk, dev = int(volumes.shape[0]), self.RESCORE_BLOCK, next(self.parameters()).device
        srt, order = torch.sort(rows)
        cuts = torch.searchsorted(srt, torch.arange(0, N + blk, blk, device=srt.device, dtype=srt.dtype)).cpu().tolist()
        outs = [score(volumes[s:s + blk], (srt[cuts[i]:cuts[i + 1]] - s).to(dev))
                for i, s in enumerate(range(0, N, blk)) if cuts[i + 1] > cuts[i]]
        got = torch.cat(outs)
        res = torch.empty_like(got)
        res[order.to(dev)] = got
        return res


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

    def __init__(self, stages=STAGES):
        """``stages``: the cascade (:data:`STAGES` -- the CNN's thresholds; the SGAN classifier hands in its own)."""
        self.last = None
        self.stages = tuple(stages)
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
        for st in self.stages:
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
            p32 = p64.to(proba.dtype)
            tied = p32.argmax(dim=1) != p64.argmax(dim=1)
            if bool(tied.any()):
                # a float64 gap below the table's own resolution: rounding made the two largest equal (argmax would take the first).
                # The float64 winner stays on top, by one unit in the last place
                r = tied.nonzero().squeeze(1)
                top = p32[r].max(dim=1).values
                p32[r, p64[r].argmax(dim=1)] = torch.nextafter(top, torch.full_like(top, 2.0))
            proba[idx] = p32
            pos += int(idx.numel())
            if pos < n and float(gs[pos]) >= max(8.0 * e6, 1e-6):
                break
        rep["rescored_float64"] += pos
        rep["observed_error_x6"] = max(rep["observed_error_x6"], e6)
