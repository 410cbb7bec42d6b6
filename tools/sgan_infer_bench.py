"""SGAN classifier inference on the fused HIP chain (csrc/sgan_infer.hip + the LeakyReLU tail of csrc/dense.hip): one JSON line.

    timeout -k 10 600 python tools/sgan_infer_bench.py [--torch | --guard [--out FILE]] [--batch 4096] [--frames 4096] [--steps 20] [--warmup 5]

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
With --guard nothing of the above runs; instead, one JSON line that is also written to --out (profiles/sgan_guard_bench.json):
  guard                   Discriminator.predict_volumes on --frames Walabot frames with label_guard off and at sgan.LABEL_GUARD, on a
                          trained-like model (decided probabilities: few rows near a tie) and on a model with no margins (the
                          N(0, 0.02) initialisation: every row is re-scored), with what the guard did (last_guard)
  x3 / x6                 microseconds per row of forward_exact("x3") and ("x6") (csrc/sgan_x3.hip + rml_dense_tail_lrelu_f32) on
                          float32 planes, at a handful of rows (8) and at 256
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


def trained_like(model, seed=1):
    """kernels ~ N(0, sqrt(2 / fan_in)) (activations of order one through the LeakyReLU layers), a last layer large enough for decided
    probabilities, non-trivial biases and BatchNorm statistics: what a trained classifier looks like to the guard"""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
                gain = 6.0 if mod is model.fc3 else 2.0 ** 0.5
                mod.weight.copy_((torch.randn(mod.weight.shape, generator=g) * (gain / mod.weight[0].numel() ** 0.5)).to(mod.weight.device))
                mod.bias.copy_((torch.randn(mod.bias.shape, generator=g) * 0.2).to(mod.bias.device))
            elif isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.weight.copy_((torch.rand(mod.weight.shape, generator=g) + 0.5).to(mod.weight.device))
                mod.bias.copy_((torch.randn(mod.bias.shape, generator=g) * 0.3).to(mod.bias.device))
    return model


def guard_bench(args):
    import torch
    import radar_ml_amd as rml
    from radar_ml_amd import sgan
    torch.manual_seed(0)
    res = {"what": "SGAN classifier margin guard", "frames": args.frames, "grid": [22, 31, 176], "planes": [3, 128, 128], "steps": args.steps,
           "label_guard": sgan.LABEL_GUARD, "device": torch.cuda.get_device_name(0)}
    v, _ = rml.synth_volumes(args.frames, 22, 31, 176, seed=7)
    for name in ("trained_like", "no_margins"):
        model = sgan.define_discriminator(device="cuda").eval()
        with torch.no_grad():
            for mod in model.modules():
                if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    mod.running_mean.normal_(0.0, 0.1)
                    mod.running_var.uniform_(0.5, 2.0)
        if name == "trained_like":
            trained_like(model)
        off = median_ms(lambda: model.predict_volumes(v, batch_size=args.batch, return_numpy=False), args.steps, args.warmup)
        on = median_ms(lambda: model.predict_volumes(v, batch_size=args.batch, return_numpy=False, label_guard=sgan.LABEL_GUARD), args.steps, args.warmup)
        rep = {k: (round(x, 9) if isinstance(x, float) else x) for k, x in model.last_guard.items()}
        res[name] = {"guard_off_ms": round(off, 4), "guard_on_ms": round(on, 4), "guard_cost": round(on / off - 1.0, 4), "last_guard": rep}
        if name == "trained_like":
            for rows in (8, 256):
                xs = [torch.rand((rows, 128, 128), device="cuda") * 2 - 1 for _ in range(3)]
                for prec in ("x3", "x6"):
                    ms = median_ms(lambda: model.forward_exact(*xs, precision=prec), args.steps, args.warmup)
                    res["%s_us_per_row_at_%d_rows" % (prec, rows)] = round(ms * 1e3 / rows, 3)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--guard", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgan_guard_bench.json"))
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.guard:
        return guard_bench(args)
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
