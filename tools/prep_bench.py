#!/usr/bin/env python3
"""Seconds for ``dnn.preprocess_data`` / ``sgan.preprocess_data`` with and without ``augment`` on a synthetic data set of the reference's
size (4 868 samples at the Walabot projection shapes 22x176 / 31x176 / 22x31, float32 planes of sparse integers 0..255), one JSON line.
With ``--host`` the same work is also timed through SciPy / Pillow / NumPy on this host (the restatement in tests/prep_common.py -- its
stage functions only, nothing of the test harness is imported --, one thread, as the reference runs it).  Times include the host half
(draws, stacking, upload, download of the result).  Every row is measured the same way: one warm-up call that is not counted, then the
best of ``--repeat`` calls; the host rows repeat ``--host-repeat`` times (default 2: a call takes seconds).

    python tools/prep_bench.py [--host] [--samples 4868] [--repeat 3] [--host-repeat 2] [--host-samples N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((22, 176), (31, 176), (22, 31))


class Args:
    def __init__(self, augment, train_split=0.8):
        self.augment, self.train_split = augment, train_split


def synth(n, seed=0):
    rng = np.random.default_rng(seed)
    planes = []
    for shape in SHAPES:
        v = rng.integers(1, 256, (n,) + shape).astype(np.float32)
        v[rng.random((n,) + shape) < 0.4] = 0.0
        planes.append(v)
    data = [tuple(p[i] for p in planes) for i in range(n)]
    labels = [("person", "dog", "cat")[k] for k in rng.choice(3, n, p=(0.55, 0.3, 0.15))]
    return data, labels, rng.random(n) < 0.5


def timed(fn, repeat, device=True):
    import torch
    sync = torch.cuda.synchronize if device else (lambda: None)
    fn()
    best = None
    for _ in range(repeat):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host", action="store_true", help="also time the SciPy / Pillow restatement on the host")
    ap.add_argument("--samples", type=int, default=4868)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-repeat", type=int, default=2)
    ap.add_argument("--host-samples", type=int, default=None, help="time the host restatement on the first N samples only (reported as host_samples)")
    a = ap.parse_args()
    import radar_ml_amd.dnn as dnn
    import radar_ml_amd.sgan as sgan
    data, labels, sup = synth(a.samples)
    out = {"tool": "prep_bench", "samples": a.samples, "shapes": [list(s) for s in SHAPES], "seconds": {}}
    for aug in (False, True):
        for keep in (True, False):
            tag = ("augment" if aug else "plain") + ("" if keep else "_resident")
            out["seconds"]["dnn_" + tag] = timed(lambda: dnn.preprocess_data(Args(aug), data, labels, rng=np.random.default_rng(1234), return_numpy=keep), a.repeat)
            out["seconds"]["sgan_" + tag] = timed(lambda: sgan.preprocess_data(Args(aug), data, labels, sup, rng=np.random.default_rng(1234), return_numpy=keep), a.repeat)
    if a.host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import prep_common as pc
        nh = a.samples if a.host_samples is None else min(a.host_samples, a.samples)
        out["host_samples"] = nh
        for aug in (False, True):
            tag = "augment" if aug else "plain"
            for name, rescale, s in (("dnn", (80, 80), None), ("sgan", (128, 128), sup)):
                out["seconds"]["host_%s_%s" % (name, tag)] = timed(
                    lambda: pc.preprocess(pc.Args(aug), data[:nh], labels[:nh], rescale, np.random.default_rng(1234), None if s is None else s[:nh]),
                    a.host_repeat, device=False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
