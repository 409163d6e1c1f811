"""bench.py's two kinds of run on a small vis_fwd workload: a plain run prints the headline line (and writes
--dump-outputs) without the instrumented extras; --full adds them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
SMALL = ["--gpus", "1", "--workload", "vis_fwd", "--batch", "2", "--steps", "2", "--warmup", "1"]


def _line(args):
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[-1])


def test_plain_run_prints_the_headline_only(tmp_path):
    d = _line(SMALL + ["--dump-outputs", str(tmp_path)])
    assert d["full"] is False and d["higher_is_better"] is True and d["unit"] == "slides/s" and d["dtype"] == "bf16"
    assert d["steps"] == 2 and d["warmup"] == 1 and abs(d["value"] - 2e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    assert not {"roofline", "cpu_baseline", "power", "check", "accuracy_vs_reference", "secondary"} & set(d)
    pred = np.load(tmp_path / "pred.npy")
    assert pred.shape == (2, 20820) and np.isfinite(pred).all()


def test_full_run_adds_the_roofline():
    d = _line(SMALL + ["--full", "--no-cpu-baseline"])
    assert d["full"] is True and d["value"] > 0
    assert d["roofline"] and d["roofline"]["kernel"] and d["roofline"]["launches_per_step"] > 0
