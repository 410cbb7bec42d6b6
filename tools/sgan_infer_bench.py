"""SGAN classifier inference on the fused HIP chain (csrc/sgan_infer.hip + the LeakyReLU tail of csrc/dense.hip): one JSON line.

    timeout -k 10 600 python tools/sgan_infer_bench.py [--torch] [--batch 4096] [--frames 4096] [--steps 20] [--warmup 5]

Seeded synthetic data at the reference's size (three 128 x 128 planes, three classes).  HIP events, medians of --steps runs after
--warmup.  Reported:
  trunk_ms, tail_ms       Discriminator.features_fused / dense_tail_fused per batch of --batch samples (bf16 planes), the samples/s of
                          the two together, and the trunk's share of the bf16 matrix-core peak at 1.6 GHz (the yardstick of DESIGN
                          3.5: 256 CUs x 4 SIMDs x 1 024 FLOP/clk), counted on the 510 MFLOP per sample the layers need -- the
                          recomputed conv1 (+25 % matrix instructions) is not counted as useful work
  predict_volumes         frames/s of Discriminator.predict_volumes for --frames frames resident on the device, at the Walabot grid
                          22 x 31 x 176 and at 64 x 64 x 128, from float32 and from uint8 volumes, and the preprocessing route of
                          each grid: "fused" (rml_dnn_preprocess_volumes) or "exact" (projection to float32 rows + the Pillow-exact
                          resize, what 64 x 64 x 128 takes at 128 x 128)
  torch                   with --torch, the comparator at the same batch in the same process: DiscriminatorTrainer.predict's inner
                          call (the plain PyTorch layers in inference mode) under float16 autocast and under bfloat16 autocast, on
                          planes already on the device
No figure here is a pass / fail gate.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = 3 * 2.0 * (64 * 64 * 128 * 9 + 32 * 32 * 64 * 1152 + 16 * 16 * 32 * 576)      # the three convolutions: 510 MFLOP
PEAK_BF16_1600 = 256 * 4 * 1024 * 1.6e9                                                            # FLOP/s at 1.6 GHz


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
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import radar_ml_amd as rml
    from radar_ml_amd import nn_common, sgan

    torch.manual_seed(0)
    nb = args.batch
    model = sgan.define_discriminator(device="cuda").eval()
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.running_mean.normal_(0.0, 0.1)
                mod.running_var.uniform_(0.5, 2.0)
    xs = [(torch.rand((nb, 128, 128), device="cuda") * 2 - 1).to(torch.bfloat16) for _ in range(3)]
    res = {"what": "SGAN classifier inference, fused HIP chain", "batch": nb, "planes": [3, 128, 128], "steps": args.steps,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        fv = model.features_fused(*xs)
        res["trunk_ms"] = round(median_ms(lambda: model.features_fused(*xs), args.steps, args.warmup), 4)
        res["tail_ms"] = round(median_ms(lambda: model.dense_tail_fused(fv), args.steps, args.warmup), 4)
        res["forward_fused_ms"] = round(median_ms(lambda: model.forward_fused(*xs), args.steps, args.warmup), 4)
    res["samples_per_s"] = round(nb / (res["forward_fused_ms"] * 1e-3), 1)
    res["trunk_samples_per_s"] = round(nb / (res["trunk_ms"] * 1e-3), 1)
    res["trunk_mflop_per_sample"] = round(FLOP_PER_SAMPLE / 1e6, 1)
    res["trunk_fraction_of_bf16_peak_at_1600MHz"] = round(FLOP_PER_SAMPLE * nb / (res["trunk_ms"] * 1e-3) / PEAK_BF16_1600, 4)

    pv = {}
    for name, grid in (("walabot_22x31x176", (22, 31, 176)), ("grid_64x64x128", (64, 64, 128))):
        v, _ = rml.synth_volumes(min(args.frames, 512), *grid, seed=7)
        pv[name + "_preprocessing"] = "fused" if nn_common.preprocess_supported(grid, (128, 128)) else "exact"
        v = v.repeat((args.frames + v.shape[0] - 1) // v.shape[0], 1, 1, 1)[:args.frames].contiguous()
        for tag, vv in (("float32", v.float()), ("uint8", v.to(torch.uint8))):
            ms = median_ms(lambda: model.predict_volumes(vv, batch_size=nb, return_numpy=False), args.steps, args.warmup)
            pv["%s_%s_frames_per_s" % (name, tag)] = round(args.frames / (ms * 1e-3), 1)
        del v
    res["predict_volumes"] = dict(pv, frames=args.frames)

    if args.torch:
        x4 = [x.float().unsqueeze(1).contiguous(memory_format=torch.channels_last) for x in xs]
        cmp = {}
        for tag, dt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
            def plain():
                with torch.no_grad(), torch.autocast("cuda", dtype=dt):
                    return torch.softmax(model(*x4).float(), dim=-1)
            ms = median_ms(plain, args.steps, args.warmup)
            cmp["plain_eval_%s_ms" % tag] = round(ms, 4)
            cmp["plain_eval_%s_samples_per_s" % tag] = round(nb / (ms * 1e-3), 1)
        cmp["fused_speedup_over_float16"] = round(cmp["plain_eval_float16_ms"] / res["forward_fused_ms"], 2)
        res["torch"] = cmp
    print(json.dumps(res))


if __name__ == "__main__":
    main()
