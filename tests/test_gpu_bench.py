"""bench.py without --full: the headline line and the dumped arrays, none of the --full legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_is_headline_only(tmp_path):
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(dump)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "coord-samples/sec fwd+bwd, 4x256 complex WIRE MLP"
    assert out["unit"] == "coord-samples/s" and out["higher_is_better"] is True
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 2 and out["warmup"] == 1
    assert out["dtype"].startswith("f32")
    assert np.isfinite(out["final_loss"])
    for leg in ("cpu_baseline", "extras", "secondary"):
        assert leg not in out, leg
    assert out["config"]["rccl_nranks"] is None
    for name in ("loss", "y", "batch_indices", "grad", "params", "adam_exp_avg", "adam_exp_avg_sq"):
        assert (dump / (name + ".npy")).exists(), name
    assert np.load(dump / "loss.npy").item() == pytest.approx(out["final_loss"], rel=1e-6)
