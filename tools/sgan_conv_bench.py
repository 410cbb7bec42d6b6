"""The SGAN discriminator's 3x3 stride-2 convolutions in training: csrc/conv_train.hip against the library (F.conv2d, i.e. MIOpen), pass by
pass and in the three-update step.  One JSON line, also written to profiles/sgan_conv_bench.json.

    timeout -k 10 900 python tools/sgan_conv_bench.py [--part kernels|step|all] [--steps 20] [--warmup 5] [--batch 256] [--rounds 2]

(a) kernels: forward, data gradient and weight gradient alone at the config-4 shapes -- 128 -> 64 channels on 129 x 129 padded planes and
    64 -> 32 on 65 x 65 -- at batch 256 and at the reference's half batch 16, float16, random data: nn_common.conv3s2 ("hip") and
    F.conv2d forward / autograd backward ("library") on the SAME tensors in the same process, medians of --steps runs after --warmup,
    HIP events; mfma_fraction = 2 N Ho Wo 9 Cin Cout flops / time / 2.5 PFLOP/s (the device's dense float16 specification).
(b) step: c + d on real + d on fake at --batch, three 128 x 128 projections, float16, HIP-graph replay, median of --steps steps, each
    figure a FRESH process, convolutions="hip" and "library" alternating, --rounds of each.
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
SHAPES = ((128, 64, 129), (64, 32, 65))
BATCHES = (256, 16)


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
    for n in BATCHES:
        for cin, cout, hp in SHAPES:
            ho = (hp - 1) // 2
            g = torch.Generator(device="cuda").manual_seed(cin + n)
            x = torch.randn((n, hp, hp, cin), device="cuda", generator=g).half().permute(0, 3, 1, 2).requires_grad_(True)
            w = (torch.randn((cout, 3, 3, cin), device="cuda", generator=g) * 0.05).half().permute(0, 3, 1, 2).requires_grad_(True)
            dz = torch.randn((n, ho, ho, cout), device="cuda", generator=g).half().permute(0, 3, 1, 2)
            assert nn_common.conv3s2_supported(x, w)
            flops = 2.0 * n * ho * ho * 9 * cin * cout
            row = {"batch": n, "cin": cin, "cout": cout, "padded_plane": hp, "gflop": round(flops / 1e9, 3)}
            for tag, op in (("hip", nn_common.conv3s2), ("library", lambda a, b: F.conv2d(a, b, None, stride=2))):
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
    """one fresh process: median ms of the three-update step"""
    import torch
    from radar_ml_amd import sgan
    torch.manual_seed(0)
    d = sgan.define_discriminator(device="cuda")
    tr = sgan.DiscriminatorTrainer(d, amp_dtype="float16", ddp=False, use_graph=True, convolutions=impl)
    x = [torch.rand((batch, 1, 128, 128), device="cuda") * 2 - 1 for _ in range(3)]
    xf = [torch.rand((batch, 1, 128, 128), device="cuda") * 2 - 1 for _ in range(3)]
    y = torch.randint(0, 3, (batch,), device="cuda")
    real, fake = torch.full((batch, 1), 0.9, device="cuda"), torch.zeros((batch, 1), device="cuda")

    def step():
        tr.train_on_batch_c(x, y, sync=False)
        tr.train_on_batch_d(x, real, sync=False)
        tr.train_on_batch_d(xf, fake, sync=False)

    ms = median_ms(step, steps, max(warmup, 5))             # the graphs are captured after three eager steps
    print(json.dumps({"impl": impl, "step_ms": round(ms, 3), "samples_per_s": round(3 * batch / (ms * 1e-3), 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("kernels", "step", "all"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import radar_ml_amd  # noqa: F401
    if args.child:
        step_child(args.child, args.batch, args.steps, args.warmup)
        return
    res = {"what": "SGAN discriminator 3x3 stride-2 convolutions in training: csrc/conv_train.hip against the library", "amp": "float16",
           "steps": args.steps, "mfma_peak_flops": MFMA_PEAK}
    if args.part in ("step", "all"):
        # before this process opens the device: every figure its own process, the two implementations alternating
        runs = []
        for _ in range(args.rounds):
            for impl in ("hip", "library"):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", impl, "--batch", str(args.batch), "--steps",
                                      str(args.steps), "--warmup", str(args.warmup)], stdout=subprocess.PIPE, timeout=600, check=True)
                runs.append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
        res["step"] = {"batch": args.batch, "updates": "c + d real + d fake, HIP-graph replay", "runs": runs}
        for impl in ("hip", "library"):
            res["step"]["%s_ms_median" % impl] = round(float(np.median([r["step_ms"] for r in runs if r["impl"] == impl])), 3)
        res["step"]["hip_over_library"] = round(res["step"]["hip_ms_median"] / res["step"]["library_ms_median"], 3)
    if args.part in ("kernels", "all"):
        import torch
        res["device"] = torch.cuda.get_device_name(0)
        res["kernels"] = kernels(args.steps, args.warmup)
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sgan_conv_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
