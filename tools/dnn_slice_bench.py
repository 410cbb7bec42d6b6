"""CNN preprocessing of target slices straight from the volumes (csrc/preprocess_slice.hip, rml_dnn_preprocess_slices) against the
composition of the calls that served slices before it: one JSON line.

    timeout -k 10 600 python tools/dnn_slice_bench.py [--frames 8192] [--targets 4] [--steps 20] [--small-steps 200]

Seeded integer volumes at the Walabot grid 22 x 31 x 176 -> 80 x 80, T targets per frame, uint8 and float32 volumes.  Two shapes:
  large   B = --frames (8 192), T = --targets (4): the batch regime
  small   B = 1, T = --targets: one scan of the live loop (predict.py:93-119)
Per shape and volume dtype, in ONE process, the two routes alternating step by step:
  slices       nn_common.preprocess_volumes(mode="slice", ijk=(B,T,3)): index check + upload, one launch
  entry        nn_common.preprocess_slices on indices already on the device: the launch alone
  composition  process_volumes(mode="slice", ijk=(B,T,3)) -> preprocess_rows: code rows for uint8 volumes, float32 rows for float32
               volumes (the staging types of the new kernel), what a caller had to write before
Then Classifier.predict_volumes(mode="slice", ijk=(B,T,3)) end to end (guard off; small shape: guard on too).
Every figure is a host clock around the call and a device synchronise: median, and the 10th / 90th percentile as the spread, in ms.
bytes_per_target: what each route moves through HBM by count (slice voxels in, rows out and in again for the composition, planes out).
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

GRID, RESCALE = (22, 31, 176), (80, 80)


def timed(fns, steps, warmup):
    """{name: {"median_ms", "p10_ms", "p90_ms"}} of the callables in ``fns``, alternating them step by step"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                "p90_ms": round(float(np.percentile(v, 90)), 4)} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--small-steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import radar_ml_amd as rml
    from radar_ml_amd import common, dnn, nn_common
    if not torch.cuda.is_available():
        raise SystemExit("dnn_slice_bench: no GPU (there is no CPU path)")
    X, Y, Z = GRID
    T = args.targets
    D = common.feature_len(X, Y, Z)
    sl, out = (X + Y) * Z + X * Y, 3 * RESCALE[0] * RESCALE[1] * 2
    res = {"what": "CNN preprocessing of target slices: one launch from the volumes vs process_volumes rows -> preprocess_rows",
           "grid": list(GRID), "rescale": list(RESCALE), "targets_per_frame": T, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around call + synchronize; median, p10, p90",
           "bytes_per_target": {"slices_u8": sl + out, "composition_u8_code_rows": sl + 2 * ((D + 127) // 128 * 128) + out,
                                "slices_f32": 4 * sl + out, "composition_f32_rows": 4 * sl + 2 * 4 * D + out}}
    torch.manual_seed(0)
    model = dnn.define_classifier(device="cuda").eval()
    rng = np.random.default_rng(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    with torch.no_grad():
        for shape, B, steps in (("large", args.frames, args.steps), ("small", 1, args.small_steps)):
            ijk = np.stack([rng.integers(0, X, (B, T)), rng.integers(0, Y, (B, T)), rng.integers(0, Z, (B, T))], axis=2).astype(np.int32)
            ijk_t, _ = common._slice_indices(ijk, B, X, Y, Z, torch.device("cuda", torch.cuda.current_device()))
            rec = {"frames": B, "rows": B * T}
            for name in ("uint8", "float32"):
                v = torch.randint(0, 256, (B, X, Y, Z), dtype=torch.uint8, device="cuda", generator=g)
                if name == "float32":
                    v = v.float()

                def composition(v=v, name=name):
                    if name == "uint8":
                        q = rml.process_volumes(v, mode="slice", ijk=ijk, scale=False, codes="only")[1]
                        return nn_common.preprocess_rows(GRID, RESCALE, codes=q)
                    return nn_common.preprocess_rows(GRID, RESCALE, feat=rml.process_volumes(v, mode="slice", ijk=ijk, scale=False))
                fns = {"slices": lambda v=v: nn_common.preprocess_volumes(v, RESCALE, mode="slice", ijk=ijk),
                       "entry": lambda v=v: nn_common.preprocess_slices(v, ijk_t, T, RESCALE),
                       "composition": composition}
                a, b = fns["slices"](), composition()
                same = all(torch.equal(x, y) for x, y in zip(a, b))
                del a, b
                r = timed(fns, steps, args.warmup)
                r["same_bits"] = bool(same)
                r["slices_over_composition"] = round(r["slices"]["median_ms"] / r["composition"]["median_ms"], 3)
                r["targets_per_s_slices"] = round(B * T / (r["slices"]["median_ms"] * 1e-3), 1)
                r["targets_per_s_composition"] = round(B * T / (r["composition"]["median_ms"] * 1e-3), 1)
                e2e = {"guard_off": lambda v=v: model.predict_volumes(v, mode="slice", ijk=ijk, label_guard=None)}
                if shape == "small":
                    e2e["guard_on"] = lambda v=v: model.predict_volumes(v, mode="slice", ijk=ijk)
                r["predict_volumes"] = timed(e2e, max(5, steps // 2), args.warmup)
                r["predict_volumes"]["targets_per_s_guard_off"] = round(B * T / (r["predict_volumes"]["guard_off"]["median_ms"] * 1e-3), 1)
                rec[name] = r
                del v, fns, e2e
                torch.cuda.empty_cache()
            res[shape] = rec
    print(json.dumps(res))


if __name__ == "__main__":
    main()
