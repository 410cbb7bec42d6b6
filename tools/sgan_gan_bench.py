"""The SGAN four-update step with the generator (sgan.train: c, d on real, generate + d on fake, g) and the generator's output-layer
kernels alone (csrc/gen.hip): one JSON line.

    timeout -k 10 600 python tools/sgan_gan_bench.py [--torch] [--batch 32] [--steps 20] [--warmup 5] [--kernel-shape 96,128,128,128]

Seeded synthetic data at the reference's sizes (three 128 x 128 projections, latent dimension 100).  Reported:
  step_ms         median over --steps of the whole four-update step at --batch, host-synchronised once per step, after --warmup steps,
                  and of its parts c_ms, d_real_ms, generate_d_fake_ms, g_ms (HIP events around each part)
  g_torch_ms      with --torch: the g update on the plain PyTorch layers under the same autocast (sgan.plain_layers), same process
  conv7           the 7x7 one-channel convolution + tanh at --kernel-shape N,H,W,C in float16: forward and backward of the kernels
                  (nn_common.conv7_tanh, mode 3) and of the library path (F.conv2d + tanh under autocast; mode 0 is the same operands
                  through the same code), medians of --steps runs, and for each pass the fraction of the HBM time of 2 N H W C bytes
                  at hbm_TBps (the device's specification, 8 TB/s)
No figure here is a pass / fail gate.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-shape", default="96,128,128,128")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import radar_ml_amd  # noqa: F401
    from radar_ml_amd import nn_common, sgan

    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    nb, half = args.batch, args.batch // 2
    d = sgan.define_discriminator(device="cuda")
    g = sgan.define_generator(device="cuda")
    tr = sgan.DiscriminatorTrainer(d, amp_dtype="float16", ddp=False)
    gan = sgan.GanTrainer(g, tr)
    x = [torch.rand((half, 1, 128, 128), device="cuda") * 2 - 1 for _ in range(3)]
    ysup = torch.randint(0, 3, (half,), device="cuda")
    yreal = torch.full((half, 1), 0.9, device="cuda")

    def part_c():
        tr.train_on_batch_c(x, ysup, sync=False)

    def part_d():
        tr.train_on_batch_d(x, yreal, sync=False)

    def part_f():
        xf, yf = sgan.generate_fake_samples(g, 100, half, rng, return_numpy=False, amp_dtype=tr.amp_dtype)
        tr.train_on_batch_d(xf, yf, sync=False)

    def part_g():
        gan.train_on_batch_g(sgan.generate_latent_points(100, nb, rng), sgan.smooth_positive_labels(np.ones((nb, 1)), rng), sync=False)

    def step():
        part_c(); part_d(); part_f(); part_g()

    res = {"what": "SGAN four-update step with the generator", "batch": nb, "amp": "float16", "steps": args.steps,
           "device": torch.cuda.get_device_name(0)}
    res["step_ms"] = round(median_ms(step, args.steps, args.warmup), 3)
    for name, fn in (("c_ms", part_c), ("d_real_ms", part_d), ("generate_d_fake_ms", part_f), ("g_ms", part_g)):
        res[name] = round(median_ms(fn, args.steps, 2), 3)
    if args.torch:
        def part_g_torch():
            with sgan.plain_layers():
                part_g()
        res["g_torch_ms"] = round(median_ms(part_g_torch, args.steps, args.warmup), 3)

    n, h, w, c = (int(v) for v in args.kernel_shape.split(","))
    conv = torch.nn.Conv2d(c, 1, 7, padding=3).cuda()
    with torch.no_grad():
        conv.weight.normal_(0.0, 0.05)
    xk = (torch.randn((n, c, h, w), device="cuda") * 0.25).half().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.randn((n, 1, h, w), device="cuda")
    hbm_ms = 2.0 * n * h * w * c / (HBM_TBPS * 1e12) * 1e3
    k = {"shape": [n, h, w, c], "hbm_TBps": HBM_TBPS, "hbm_ms": round(hbm_ms, 4)}

    def lib_fwd():
        with torch.autocast("cuda", dtype=torch.float16):
            return torch.tanh(F.conv2d(xk, conv.weight, conv.bias, padding=3))

    for tag, fwd in (("kernel", lambda: nn_common.conv7_tanh(xk, conv, mode=3)), ("library", lib_fwd)):
        with torch.no_grad():
            k[tag + "_forward_ms"] = round(median_ms(fwd, args.steps, args.warmup), 4)
        y = fwd()
        dyt = dy.to(y.dtype)

        def bwd():
            torch.autograd.grad(y, [xk, conv.weight, conv.bias], dyt, retain_graph=True)
        k[tag + "_backward_ms"] = round(median_ms(bwd, args.steps, args.warmup), 4)
        del y
    for p in ("forward", "backward"):
        k["kernel_%s_hbm_fraction" % p] = round(hbm_ms / k["kernel_%s_ms" % p], 3)
        k["library_%s_hbm_fraction" % p] = round(hbm_ms / k["library_%s_ms" % p], 3)
    res["conv7"] = k
    print(json.dumps(res))


if __name__ == "__main__":
    main()
