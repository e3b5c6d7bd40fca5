"""GPU: the plain `bench.py` run at a tiny size — one JSON line with the headline only, exactly --steps timed steps, and
--dump-outputs writing the last timed step's loss / predictions, the same from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--clips", "1", "--hw", "40",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs_repeat(tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for res in (a, b):
        assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0.0
        assert res["unit"] == "clips/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
        assert abs(res["value"] - 1e3 / res["ms_per_step"]) <= 1e-6 * res["value"]      # 1 clip per step
        assert not {"roofline", "parity", "cpu_baseline", "bf16_path", "native_40x40_loop", "dropin_path"} & set(res)
    for name, shape in (("loss", (1,)), ("pred", (16,))):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and x.shape == shape and np.isfinite(x).all()
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6)
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")[0]) - a["config"]["final_loss"]) <= 1e-6
