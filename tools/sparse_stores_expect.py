#!/usr/bin/env python3
"""Bytes one k_project_wave launch of the headline pipeline should write with RML_OPT_SPARSE_STORES on, set against what a PMC run
measured (profiles/sparse_stores_pmc.txt):

    python tools/pmc_kernels.py --match k_project_wave --counters WRITE_SIZE -- python bench.py --gpus 1 --steps 2 --warmup 1 > pmc.txt
    python tools/sparse_stores_expect.py [pmc.txt]

Per chunk of 8 192 bench frames (64x64x128, bench.py's seed): the occupancy words rml_project_occupancy returns in the pipeline's
kernel configuration; expected = 128 B x set bits + per frame the padding line (128 B: the row stride is D + 128), the statistics
(16 B) and the words (4 B each).  Prints one JSON line per chunk, the means, and -- with a pmc_kernels.py output file -- the
measured write_bytes beside them."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import radar_ml_amd as rml                     # noqa: E402
from radar_ml_amd import _lib                  # noqa: E402
import sparse_rows_common as S                 # noqa: E402

X, Y, Z = 64, 64, 128
CH, CHUNKS, SEED = 8192, 8, 1234


def main():
    D = S.feature_len((X, Y, Z))
    KT = (D + 127) // 128
    _lib.set_option("project_share_cu", 1)
    rows = []
    for c in range(CHUNKS):
        V, _ = rml.synth_volumes(CH, X, Y, Z, seed=SEED, frame0=c * CH, device="cuda:0")
        q, occ = S.project_occupancy(torch, _lib, V, (X, Y, Z))
        bits = int(np.unpackbits(occ.view(np.uint8)).sum())
        per_frame = 128 + 16 + 4 * occ.shape[1]
        rows.append({"chunk": c, "kernel_wrote_words": bool((occ != 0xFFFFFFFF).any()), "set_bits": bits, "lines": KT * CH,
                     "occupied_share": round(bits / (KT * CH), 4), "expected_bytes": 128 * bits + per_frame * CH,
                     "whole_rows_bytes": 128 * KT * CH + per_frame * CH})
        del V
    for r in rows:
        print(json.dumps(r))
    out = {"mean_expected_bytes": float(np.mean([r["expected_bytes"] for r in rows])),
           "mean_whole_rows_bytes": float(np.mean([r["whole_rows_bytes"] for r in rows]))}
    if len(sys.argv) > 1:
        for line in open(sys.argv[1]):
            if line.startswith("{") and "write_bytes" in line:
                e = json.loads(line)
                if e.get("write_bytes"):
                    out["measured_write_bytes"] = e["write_bytes"]
                    out["measured_over_expected"] = round(e["write_bytes"] / out["mean_expected_bytes"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
