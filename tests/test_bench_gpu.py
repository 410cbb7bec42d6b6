"""A plain bench.py run (no --full) on a real GPU: the contract line alone, --steps timed steps, and --dump-outputs writing what the last
timed step returned -- the same arrays, to the last bit, from two runs with the same arguments."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(dump, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--frames", "2048", "--train", "1500", "--dump-outputs", dump], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                    # no {"doc": ...} line without --full
    return json.loads(lines[0])


def test_plain_bench_prints_the_contract_line_and_dumps_the_last_step(tmp_path):
    line = _plain(str(tmp_path / "a"), 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 2048 / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    assert line["cpu_baseline"] is None and "parity_gate" not in line["summary"]      # what --full measures is not run
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(d) == ["dec_ovo", "dec_ovr", "label_calib", "label_vote", "proba"]
    assert all(v.dtype in (np.float32, np.float64) and len(v) == 2048 for v in d.values())
    assert zlib.crc32(d["label_calib"].astype(np.int32).tobytes()) == line["labels_crc32"]
    np.testing.assert_allclose(d["proba"].sum(axis=1), 1.0, rtol=0, atol=1e-9)
    assert np.array_equal(d["label_calib"], d["proba"].argmax(axis=1).astype(np.float64))
    # same arguments but the number of steps: the same inputs, model and outputs
    line2 = _plain(str(tmp_path / "b"), 2)
    assert line2["steps"] == 2 and line2["labels_crc32"] == line["labels_crc32"]
    for k, v in d.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))), k
