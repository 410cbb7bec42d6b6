"""Shared by test_dnn_guard_cpu.py and test_dnn_guard_gpu.py: a stand-in for the margin guard's device operations, written from the
contract of rml_dnn_top2_gap / rml_dnn_guard_apply in include/radarml.h with plain torch on the tensors' own device -- the CPU tests
drive the policy (radar-ml_amd/dnn_guard.py MarginGuard) with it, the GPU tests hold csrc/guard.hip against it."""
import importlib

import torch


def top2_gap(p):
    """gap[r] = largest - second largest of row r, float32; 0 for a row that holds a non-finite value (it counts as a tie)"""
    p = p.float()
    fin = torch.isfinite(p).all(dim=1)
    srt = torch.sort(torch.where(fin[:, None], p, torch.zeros_like(p)), dim=1, descending=True).values
    return torch.where(fin, srt[:, 0] - srt[:, 1], torch.zeros_like(srt[:, 0]))


def guard_apply(proba, rows, fresh, thr_close, gap):
    """proba[rows[i]] <- fresh[i]; returns (stats[0]: largest |old - new| over the rows where both are finite, as a float32 tensor;
    stats[1]: rows whose NEW top-2 gap is below float32(thr_close); close: that test per row, uint8); gap[rows] <- +inf when given"""
    old = proba[rows].clone()
    fin = torch.isfinite(old).all(dim=1) & torch.isfinite(fresh).all(dim=1)
    d = torch.where(fin, torch.nan_to_num(old - fresh).abs().max(dim=1).values, torch.zeros_like(old[:, 0]))
    proba[rows] = fresh
    close = top2_gap(fresh) < torch.tensor(thr_close, dtype=torch.float32, device=fresh.device)
    if gap is not None:
        gap[rows] = float("inf")
    err = d.max() if d.numel() else torch.zeros((), dtype=torch.float32)
    return err.float(), int(close.sum()), close.to(torch.uint8)


def host_ops():
    """A GuardOps made of the two functions above that writes down every call: .calls = [("gaps",) | ("candidates", thr, rows) |
    ("apply", rows, thr_close, gap given)]."""
    dnn_guard = importlib.import_module("radar_ml_amd.dnn_guard")

    class HostOps(dnn_guard.GuardOps):
        def __init__(self):
            self.calls = []

        def gaps(self, proba):
            self.calls.append(("gaps",))
            return top2_gap(proba)

        def candidates(self, gap, thr):
            cand = dnn_guard.GuardOps.candidates(self, gap, thr)
            self.calls.append(("candidates", thr, [] if cand is None else cand.tolist()))
            return cand

        def apply(self, proba, rows, fresh, thr_close, gap):
            self.calls.append(("apply", rows.tolist(), thr_close, gap is not None))
            err, still, close = guard_apply(proba, rows, fresh, thr_close, gap)
            return float(err), still, close

    return HostOps()
