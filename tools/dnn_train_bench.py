"""Training step of the multi-view CNN on the GPU (Classifier.fit: rml_dnn_train_step + rml_adam_step): one JSON line.

    python tools/dnn_train_bench.py [--torch] [--samples 3894] [--steps 50] [--warmup 10]

Seeded synthetic data: --samples training samples of three 80 x 80 planes in three classes (3 894 = 80 % of the reference's 4 868,
train-results/dnn/train.log:13) and a quarter as many validation samples.  Reported:
  step_ms        median over --steps of one update at B = 64 as fit queues it (rml_dnn_train_step + rml_adam_step on resident rows,
                 no read-back), HIP events, after --warmup updates
  call_ms        the same update as train_on_batch pays it: rows uploaded, accumulators read back, host-synchronised
  epoch_ms       one epoch over all samples in batches of 64, the validation pass and the epoch's one read of device memory included
                 (wall time, host-synchronised, the data resident)
  torch_step_ms  with --torch: the plain PyTorch float32 step of the same module (Classifier.logits + autograd + torch.optim.Adam,
                 class-weighted cross-entropy) on batches of 64 gathered from the same resident data, in this process on this GPU
No figure here is a pass / fail gate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 80
C = 3
B = 64


def synth(n, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, size=n)
    xs = []
    for v in range(3):
        a = rng.normal(-0.8, 0.1, (n, H, W)) + 0.3 * np.sin((1 + y)[:, None, None] * np.arange(W)[None, None, :] / (5.0 + v))
        xs.append(np.clip(a, -1, 1).astype(np.float32))
    return xs, y


def median_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--samples", type=int, default=3894)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    import radar_ml_amd.dnn as D
    torch.manual_seed(0)
    xs, y = synth(args.samples, 1)
    vx, vy = synth(max(args.samples // 4, 1), 2)
    cw = {0: 5.48, 1: 1.26, 2: 1.0}
    res = {"tool": "dnn_train_bench", "planes": [H, W], "batch": B, "classes": C, "samples": int(args.samples), "val_samples": int(len(vy)),
           "device": torch.cuda.get_device_name(0)}
    m = D.define_classifier(n_classes=C).compile()
    job = m._job(xs, y, (vx, vy), cw, B, trusted=True)
    rows = np.arange(B, dtype=np.int32)
    rng = np.random.default_rng(0)
    D._fit_epoch(m, job, rng.permutation(args.samples).astype(np.int32))       # upload + warm-up
    fit = D._DeviceFit(m, job)
    drows = torch.from_numpy(rng.permutation(args.samples).astype(np.int32)[:B]).cuda()
    with torch.no_grad():
        res["step_ms"] = round(median_ms(lambda: fit.train(drows, 0, B), args.steps, args.warmup), 4)
    step_job = m._job([a[:B] for a in xs], y[:B], None, cw, B, trusted=True)
    res["call_ms"] = round(median_ms(lambda: D._fit_epoch(m, step_job, rows), args.steps, args.warmup), 4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D._fit_epoch(m, job, rng.permutation(args.samples).astype(np.int32))
    torch.cuda.synchronize()
    res["epoch_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    res["steps_per_epoch"] = -(-args.samples // B)
    if args.torch:
        ref = D.define_classifier(n_classes=C)
        ref.train()
        opt = torch.optim.Adam(ref.parameters(), lr=0.0002, betas=(0.5, 0.999), eps=1e-7)
        dx = [torch.from_numpy(a).cuda().unsqueeze(1) for a in xs]
        dy = torch.from_numpy(y).cuda()
        w = torch.tensor([cw[c] for c in range(C)], dtype=torch.float32, device="cuda")
        idx = torch.from_numpy(rows.astype(np.int64)).cuda()

        def torch_step():
            opt.zero_grad(set_to_none=True)
            yb = dy[idx]
            z = ref.logits(*[a[idx] for a in dx])
            loss = (w[yb] * torch.nn.functional.cross_entropy(z, yb, reduction="none")).sum() / B
            loss.backward()
            opt.step()
        res["torch_step_ms"] = round(median_ms(torch_step, args.steps, args.warmup), 4)
        res["speedup"] = round(res["torch_step_ms"] / res["step_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
