"""bench.py as the driver runs it: a plain run prints the headline line and
nothing that needs a run of its own (those are behind --full), --steps sets
the number of timed steps, and --dump-outputs writes the last timed step's
span records as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dump(tmp_path):
    out = tmp_path / "b.json"
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--scale", "0.02", "--dump-outputs", str(dump), "--out", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line == json.loads(out.read_text())
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "Gbases/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    bp = line["config"]["genome_bp"]
    # value = bases per step / ms_per_step (the line rounds ms_per_step to 1 us: 1 % at 0.05 ms)
    assert abs(line["value"] - bp / (line["ms_per_step"] * 1e-3) / 1e9) <= 1e-2 * line["value"]
    # what takes runs of its own is behind --full
    for key in ("cpu_baseline", "parity_sample", "table_equal_host", "visits_path", "host_path", "configs",
                "end_to_end"):
        assert line[key] is None, key
    assert "host_multi" not in line and "count_ms" not in line["setup_ms"]
    pos = np.load(dump / "pos.npy")
    score = np.load(dump / "score.npy")
    assert sorted(os.listdir(dump)) == ["pos.npy", "score.npy"]
    assert pos.dtype == np.float64 and score.dtype == np.float64
    assert pos.shape == (3, line["regions"]) and score.shape == (2, line["regions"])
    assert np.array_equal(pos, np.round(pos)) and np.all(pos[2] >= pos[1])
