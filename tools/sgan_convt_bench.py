"""The SGAN generator's 4x4 stride-2 transposed convolutions in training: csrc/convt_train.hip against the library
(F.conv_transpose2d, i.e. MIOpen), pass by pass, in the g update and in the four-update step.  One JSON line, also written to
profiles/sgan_convt_bench.json.

    timeout -k 10 900 python tools/sgan_convt_bench.py [--part kernels|step|all] [--steps 20] [--warmup 5] [--batch 32] [--rounds 2]

(a) kernels: forward, data gradient and weight gradient alone on the generator's four layers -- 128 -> 128 channels on 8 x 8, 16 x 16,
    32 x 32 and 64 x 64 input planes -- at batch 32, and the last at batch 96 (the three branches' worth), float16, random data:
    nn_common.convt4s2 ("hip") and F.conv_transpose2d forward / autograd backward ("library") on the SAME tensors in the same process,
    medians of --steps runs after --warmup, HIP events; mfma_fraction = 2 N H W 16 Cin Cout flops / time / 2.5 PFLOP/s (the device's
    dense float16 specification).
(b) step: the g update alone and the whole four-update step (c, d on real, generate + d on fake, g) at --batch, three 128 x 128
    projections, float16, median of --steps after --warmup, host-synchronised once per step; each figure a FRESH process, the
    generator's convolutions="hip" and "library" alternating, --rounds of each.  The discriminator's convolutions are "library" in
    both, so only the generator's layers differ.
No figure here is a pass / fail gate.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_PEAK = 2.5e15
SHAPES = ((32, 8), (32, 16), (32, 32), (32, 64), (96, 64))      # (batch, input plane edge)
CH = 128


def median_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def kernels(steps, warmup):
    import torch
    import torch.nn.functional as F
    from radar_ml_amd import nn_common
    rows = []
    for n, h in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(n + h)
        x = torch.randn((n, h, h, CH), device="cuda", generator=g).half().permute(0, 3, 1, 2).requires_grad_(True)
        w = (torch.randn((CH, 4, 4, CH), device="cuda", generator=g) * 0.05).half().permute(0, 3, 1, 2).requires_grad_(True)
        dz = torch.randn((n, 2 * h, 2 * h, CH), device="cuda", generator=g).half().permute(0, 3, 1, 2)
        assert nn_common.convt4s2_supported(x, w)
        flops = 2.0 * n * h * h * 16 * CH * CH
        row = {"batch": n, "input_plane": h, "gflop": round(flops / 1e9, 3)}
        for tag, op in (("hip", nn_common.convt4s2), ("library", lambda a, b: F.conv_transpose2d(a, b, None, stride=2, padding=1))):
            with torch.no_grad():
                t = {"forward": median_ms(lambda: op(x, w), steps, warmup)}
            # one gradient at a time: the graph is built with only that input requiring a gradient (a custom autograd.Function sees
            # what its inputs require, not which of them autograd.grad was asked for)
            xd, wd = x.detach(), w.detach()
            z = op(x, wd)
            t["dgrad"] = median_ms(lambda: torch.autograd.grad(z, [x], dz, retain_graph=True), steps, warmup)
            z = op(xd, w)
            t["wgrad"] = median_ms(lambda: torch.autograd.grad(z, [w], dz, retain_graph=True), steps, warmup)
            del z
            for k, v in t.items():
                row["%s_%s_ms" % (tag, k)] = round(v, 4)
                row["%s_%s_mfma_fraction" % (tag, k)] = round(flops / (v * 1e-3) / MFMA_PEAK, 4)
        for k in ("forward", "dgrad", "wgrad"):
            row["hip_over_library_%s" % k] = round(row["hip_%s_ms" % k] / row["library_%s_ms" % k], 3)
        rows.append(row)
        del x, w, dz
        torch.cuda.empty_cache()
    return rows


def step_child(impl, batch, steps, warmup):
    """one fresh process: median ms of the g update and of the four-update step"""
    import torch
    from radar_ml_amd import sgan
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    half = batch // 2
    d = sgan.define_discriminator(device="cuda")
    g = sgan.define_generator(device="cuda", convolutions=impl)
    tr = sgan.DiscriminatorTrainer(d, amp_dtype="float16", ddp=False)
    gan = sgan.GanTrainer(g, tr)
    assert g.conv_impl == impl
    x = [torch.rand((half, 1, 128, 128), device="cuda") * 2 - 1 for _ in range(3)]
    ysup = torch.randint(0, 3, (half,), device="cuda")
    yreal = torch.full((half, 1), 0.9, device="cuda")

    def part_g():
        gan.train_on_batch_g(sgan.generate_latent_points(100, batch, rng), sgan.smooth_positive_labels(np.ones((batch, 1)), rng), sync=False)

    def step():
        tr.train_on_batch_c(x, ysup, sync=False)
        tr.train_on_batch_d(x, yreal, sync=False)
        xf, yf = sgan.generate_fake_samples(g, 100, half, rng, return_numpy=False, amp_dtype=tr.amp_dtype)
        tr.train_on_batch_d(xf, yf, sync=False)
        part_g()

    step_ms = median_ms(step, steps, warmup)
    g_ms = median_ms(part_g, steps, 2)
    print(json.dumps({"impl": impl, "step_ms": round(step_ms, 3), "g_ms": round(g_ms, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("kernels", "step", "all"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import radar_ml_amd  # noqa: F401
    if args.child:
        step_child(args.child, args.batch, args.steps, args.warmup)
        return
    res = {"what": "SGAN generator 4x4 stride-2 transposed convolutions in training: csrc/convt_train.hip against the library",
           "amp": "float16", "steps": args.steps, "mfma_peak_flops": MFMA_PEAK}
    if args.part in ("step", "all"):
        # before this process opens the device: every figure its own process, the two implementations alternating
        runs = []
        for _ in range(args.rounds):
            for impl in ("hip", "library"):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", impl, "--batch", str(args.batch), "--steps",
                                      str(args.steps), "--warmup", str(args.warmup)], stdout=subprocess.PIPE, timeout=300, check=True)
                runs.append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
        res["step"] = {"batch": args.batch, "updates": "c + d real + generate + d fake + g, eager", "runs": runs}
        for key in ("step_ms", "g_ms"):
            for impl in ("hip", "library"):
                res["step"]["%s_%s_median" % (impl, key)] = round(float(np.median([r[key] for r in runs if r["impl"] == impl])), 3)
            res["step"]["hip_over_library_%s" % key] = round(res["step"]["hip_%s_median" % key] / res["step"]["library_%s_median" % key], 3)
    if args.part in ("kernels", "all"):
        import torch
        res["device"] = torch.cuda.get_device_name(0)
        res["kernels"] = kernels(args.steps, args.warmup)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sgan_convt_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
