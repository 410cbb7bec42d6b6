"""SGAN generator inference on the fused HIP chain (csrc/gen_infer.hip + the forward of csrc/gen.hip) against the plain PyTorch layers
in inference mode: one JSON line, printed and written to profiles/gen_infer_bench.json.

    timeout -k 10 900 python tools/gen_infer_bench.py [--batches 16,100,4096] [--steps 20] [--warmup 5] [--dtype bfloat16]

The generator at the default size (latent 100, 128 channels, 8 x 8 -> 128 x 128, three branches), seeded weights.  HIP events, medians
of --steps runs after --warmup, the two arms interleaved run by run in one process.  Reported:
  predict                 per batch size: Generator.predict(fused=True) and Generator.predict(fused=False) under the same autocast type
                          (return_numpy=False, latent points on the device), their ratio, and the fused samples/s
  gen_up                  per layer (input plane H): one rml_gen_up_forward launch at --layer-batch samples, its share of the bf16
                          matrix peak at 1.6 GHz (256 CUs x 4 SIMDs x 1 024 FLOP/clk, the yardstick of DESIGN 3.5) counted on
                          2 (2H 2W) 4 C^2 flops per sample
  train_piece             the "generate + d on fake" piece of sgan.train's step at the loop's half batch: generate_fake_samples +
                          train_on_batch_d(sync=False), with and without fused generation, float16 autocast as in the loop
No figure here is a pass / fail gate.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16_1600 = 256 * 4 * 1024 * 1.6e9            # FLOP/s at 1.6 GHz
C = 128


def interleaved_ms(fns, steps, warmup):
    """median HIP-event time of every callable of ``fns`` (a dict), one run of each per round"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,100,4096")
    ap.add_argument("--layer-batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float16"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_infer_bench.json"))
    args = ap.parse_args()
    import torch
    from radar_ml_amd import _lib, sgan

    torch.manual_seed(0)
    dt = getattr(torch, args.dtype)
    gen = sgan.define_generator(device="cuda").eval()
    with torch.no_grad():
        for mod in gen.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0.0, 0.1)
                mod.running_var.uniform_(0.5, 2.0)
    res = {"what": "SGAN generator inference, fused HIP chain against the plain eval layers", "dtype": args.dtype, "steps": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "predict": {}, "gen_up": {}}

    for nb in (int(v) for v in args.batches.split(",")):
        z = torch.randn((nb, 100), device="cuda")
        ms = interleaved_ms({"fused": lambda: gen.predict(z, return_numpy=False, amp_dtype=dt, fused=True),
                             "plain": lambda: gen.predict(z, return_numpy=False, amp_dtype=dt)}, args.steps, args.warmup)
        res["predict"][str(nb)] = {"fused_ms": round(ms["fused"], 4), "plain_ms": round(ms["plain"], 4),
                                   "plain_over_fused": round(ms["plain"] / ms["fused"], 3),
                                   "fused_samples_per_s": round(nb / (ms["fused"] * 1e-3), 1)}
        print("predict, batch %d: %s" % (nb, res["predict"][str(nb)]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    lib, ctx = _lib.load(), _lib.context(torch.device("cuda", 0))
    pk = gen.generator_packs(dt)
    nl = args.layer_batch
    for l in range(gen.n_up):
        H = gen.base << l
        x = torch.randn((nl, H, H, C), device="cuda").to(dt)
        y = torch.empty((nl, 2 * H, 2 * H, C), dtype=dt, device="cuda")
        wt, bias = pk["up_wt"][0, l], pk["up_bias"][0, l]

        def up():
            _lib.check(lib.rml_gen_up_forward(ctx, _lib.ptr(x), 1 if dt == torch.bfloat16 else 0, nl, H, H, C, _lib.ptr(wt), _lib.ptr(bias),
                                              _lib.ptr(y), _lib.stream_ptr(None)), "rml_gen_up_forward")
        ms = interleaved_ms({"up": up}, args.steps, args.warmup)["up"]
        flop = 2.0 * (2 * H) * (2 * H) * 4 * C * C * nl
        res["gen_up"]["H%d" % H] = {"batch": nl, "ms": round(ms, 4), "tflops": round(flop / (ms * 1e-3) / 1e12, 2),
                                    "fraction_of_bf16_peak_at_1600MHz": round(flop / (ms * 1e-3) / PEAK_BF16_1600, 4)}

    # the "generate + d on fake" piece of the loop's step (sgan.py:531-532), half batch 16, float16 autocast as sgan.train runs it
    disc = sgan.define_discriminator(device="cuda")
    trainer = sgan.DiscriminatorTrainer(disc, amp_dtype="float16", ddp=False)
    rng = np.random.default_rng(0)

    def piece(fused):
        def run():
            if fused:
                xf, yf = sgan.generate_fake_samples(gen, 100, 16, rng, return_numpy=False, amp_dtype=trainer.amp_dtype, fused=True)
            else:
                xf, yf = sgan.generate_fake_samples(gen, 100, 16, rng, return_numpy=False, amp_dtype=trainer.amp_dtype)
            trainer.train_on_batch_d(xf, yf, sync=False)
        return run
    ms = interleaved_ms({"fused": piece(True), "plain": piece(False)}, args.steps, args.warmup)
    res["train_piece"] = {"half_batch": 16, "fused_generate_ms": round(ms["fused"], 4), "plain_generate_ms": round(ms["plain"], 4),
                          "plain_over_fused": round(ms["plain"] / ms["fused"], 3)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(line + "\n")


if __name__ == "__main__":
    main()
