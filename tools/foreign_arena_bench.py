#!/usr/bin/env python3
"""Volumes from a foreign arena (20x28x160) classified by a model of the Walabot geometry (22x31x176, D = 10 010): the fused call
(``decide_volumes(proj_zoom=...)`` -> rml_project_zoom_svm) beside what the library offered before it, at both grains.

    python tools/foreign_arena_bench.py [--frames 65536] [--svs 2281] [--repeats 5] [--rows-only] [--out profiles/foreign_arena_bench.json]

Batch: frames/s of the fused call and of the composition process_volumes at the source grid -> planes -> rml_zoom_features (k_zoom)
-> _decide, float32 and uint8 volumes.  Latency: host clock of ONE target (mode slice, device-resident volume, predict.py:98-119)
through the fused call, and through process_samples(proj_zoom) + predict_proba with the planes taken to the host.
``--rows-only``: rml_project_zoom alone (volumes -> zoomed rows) beside the composition without its SVM, and k_zoom_rows with the
planes of a row together / one after the other (RML_OPT_ZOOM_ROWS 1 / 2).

Every figure: two warm-up calls, then ``--repeats`` timed calls per variant, the variants ALTERNATING inside one process (the host is
shared), each call ended by a device synchronise; median, minimum and maximum are reported.  Prints one JSON line and merges it
into ``--out``.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRC, DST = (20, 28, 160), (22, 31, 176)


def alternate(variants, repeats, sync, warmup=2):
    """{name: seconds per call [repeats]} with the variants interleaved"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    sync()
    ts = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            sync()
            ts[k].append(time.perf_counter() - t0)
    return ts


def rate(ts, frames):
    r = sorted(frames / t for t in ts)
    return {"frames_per_s_median": round(float(np.median(r))), "min": round(r[0]), "max": round(r[-1])}


def micros(ts):
    u = np.array(ts) * 1e6
    return {"p50_us": round(float(np.percentile(u, 50)), 1), "min_us": round(float(u.min()), 1), "p99_us": round(float(np.percentile(u, 99)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--svs", type=int, default=2281, help="support vectors (bench.py's fitted Walabot model has about this many)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--latency-iters", type=int, default=200)
    ap.add_argument("--rows-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foreign_arena_bench.json"))
    a = ap.parse_args()
    import torch
    import radar_ml_amd as rml
    from radar_ml_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("tools/foreign_arena_bench.py measures on the GPU: no HIP device is visible")
    lib = _lib.load()
    sync = torch.cuda.synchronize
    X, Y, Z = SRC
    B, M = a.frames, a.svs
    z = rml.calc_proj_zoom(DST[0], DST[1], DST[2], X, Y, Z)
    shapes = rml.zoom_out_shapes(X, Y, Z, z)
    D = sum(h * w for h, w in shapes)
    assert D == rml.feature_len(*DST) == 10010
    V32, _ = rml.synth_volumes(B, X, Y, Z, seed=3)
    V8 = V32.to(torch.uint8)
    dev = V32.device
    ctx = _lib.context(dev)
    arr = (C.c_int32 * 6)(*[v for s in shapes for v in s])
    feat = torch.empty((B, D), dtype=torch.float32, device=dev)

    def rows_fused(V):
        return rml.process_volumes(V, mode="max", scale=True, out=feat, proj_zoom=z)

    def rows_composed(V):
        # what the library offered before: rows at the source grid -> contiguous planes -> rml_zoom_features (k_zoom)
        at = rml.process_volumes(V, mode="max", scale=False)
        xz = at[:, :X * Z].contiguous(); yz = at[:, X * Z:X * Z + Y * Z].contiguous(); xy = at[:, X * Z + Y * Z:].contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.rml_zoom_features(ctx, _lib.ptr(xz), _lib.ptr(yz), _lib.ptr(xy), B, X, Y, Z, C.cast(arr, C.c_void_p), 255.0, 7,
                                             _lib.ptr(feat), D, _lib.stream_ptr(dev)), "rml_zoom_features")
        return feat

    res = {"source_grid": list(SRC), "model_grid": list(DST), "D": D, "frames": B, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0)}
    if a.rows_only:
        def knob(v, V):
            def run():
                with _lib.options(zoom_rows=v):
                    rows_fused(V)
            return run
        out = {}
        for tag, V in (("float32", V32), ("uint8", V8)):
            ts = alternate({"rml_project_zoom": lambda V=V: rows_fused(V), "k_zoom_rows planes together": knob(1, V),
                            "k_zoom_rows plane by plane": knob(2, V), "source rows -> planes -> rml_zoom_features": lambda V=V: rows_composed(V)},
                           a.repeats, sync)
            out[tag] = {k: rate(t, B) for k, t in ts.items()}
            assert torch.equal(rows_fused(V).clone(), rows_composed(V))          # the same rows, bit for bit
        res["rows_only"] = out
        key = "rows_only"
    else:
        # the model: M zoomed rows as support vectors (off the code grid, as a model trained on zoomed projections is)
        rng = np.random.default_rng(0)
        Vm, _ = rml.synth_volumes(M, X, Y, Z, seed=11)
        sv = rml.process_volumes(Vm, mode="max", scale=True, proj_zoom=z).cpu().numpy().astype(np.float64)
        ns = np.array([M // 3, M // 3, M - 2 * (M // 3)], dtype=np.int32)
        svc = rml.GpuSVC(sv, rng.uniform(-1, 1, (2, M)), np.array([0.1, -0.2, 0.3]), ns, 0.01, np.arange(3),
                         calib_a=np.array([-1.0, -1.1, -0.9]), calib_b=np.array([0.0, 0.1, -0.1]))
        cal = rml.GpuCalibratedClassifier(svc)
        batch = {}
        for tag, V in (("float32", V32), ("uint8", V8)):
            ts = alternate({"decide_volumes(proj_zoom)": lambda V=V: svc.decide_volumes(V, mode="max", scale=True, proj_zoom=z),
                            "source rows -> planes -> rml_zoom_features -> _decide": lambda V=V: svc._decide(rows_composed(V), want_proba=True)},
                           a.repeats, sync)
            batch[tag] = {k: rate(t, B) for k, t in ts.items()}
            fused = svc.decide_volumes(V, mode="max", scale=True, proj_zoom=z)
            assert torch.equal(fused["dec_ovo"], svc._decide(rows_composed(V), want_proba=True)[0])
        res["batch"] = batch
        # one target per call (predict.py:98-119), the raw image resident on the device
        v1 = V32[:1].contiguous()
        i, j, k = X // 2, Y // 2, Z // 3
        ijk1 = torch.tensor([[i, j, k]], dtype=torch.int32, device=dev)

        def one_fused():
            return svc.decide_volumes(v1, mode="slice", ijk=ijk1, scale=True, validate_ijk=False, proj_zoom=z)["proba"]

        def one_today():
            f = v1[0]
            planes = (f[:, j, :].cpu().numpy(), f[i, :, :].cpu().numpy(), f[:, :, k].cpu().numpy())
            return cal.predict_proba(rml.process_samples([planes], proj_zoom=z, scale=True))

        ts = alternate({"decide_volumes(mode='slice', proj_zoom), B=1": one_fused,
                        "planes to the host -> process_samples(proj_zoom) -> predict_proba": one_today}, a.latency_iters, sync, warmup=10)
        res["latency_one_target"] = {k2: micros(t) for k2, t in ts.items()}
        np.testing.assert_allclose(one_fused().cpu().numpy(), one_today(), rtol=0, atol=1e-12)
        key = "decide"
    line = json.dumps(res)
    print(line)
    merged = {}
    if os.path.exists(a.out):
        try:
            merged = json.load(open(a.out))
        except ValueError:
            merged = {}
    merged[key] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
