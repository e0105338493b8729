"""-m gpu: a plain `bench.py` run -- set-up, warm-up, the timed steps, the headline line -- and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--nodes", "20000", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "graphs/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32"
    # what only --full measures is absent from a plain run
    assert not {"kernels", "roofline", "edge_scatter", "eager_ms_per_step", "cpu_baseline"} & set(d)

    loc, vloc, loss = (np.load(tmp_path / f"{n}.npy") for n in ("loc", "vloc", "loss"))
    assert loc.shape == (20000, 3) and vloc.shape == (1, 3, 16) and loss.shape == ()
    assert loc.dtype == vloc.dtype == loss.dtype == np.float32
    assert np.isfinite(loc).all() and np.isfinite(vloc).all()
    assert float(loss) == pytest.approx(d["config"]["loss"], rel=1e-6)
    grads = sorted(f for f in os.listdir(tmp_path) if f.startswith("grad."))
    assert grads and all(np.isfinite(np.load(tmp_path / f)).all() for f in grads)
