"""bench.py's plain line and --dump-outputs on one GPU: the plain run times exactly --steps steps and prints only the headline
fields (the roofline, the other arithmetic, configs and cpu_baseline are --full's), and two runs with the same arguments dump
the same outputs.  Each run is a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--model", "efficientnet-b0", "--batch", "4", "--size", "128"]


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        assert f.endswith(".npy"), f
        out[f[:-4]] = np.load(os.path.join(d, f), allow_pickle=False)
    return out


def test_plain_line_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench("--dump-outputs", str(a))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "images/sec" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 4) < 1e-6 * 4     # batch 4: images/sec x s/step = 4
    for k in ("roofline", "fp32_mfma", "split_mfma", "configs", "cpu_baseline"):
        assert k not in d, k
    got = _load(a)
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert all(np.isfinite(v).all() for v in got.values())
    for k, v in d["losses"].items():
        assert float(got[k]) == float(v), k                     # the dump holds the line's last step
    assert "params" in got and got["params"].ndim == 1 and got["params"].size > 1_000_000
    _bench("--dump-outputs", str(b))
    again = _load(b)
    assert sorted(again) == sorted(got)
    for k in got:                                               # same arguments, same inputs: the same step twice
        np.testing.assert_allclose(again[k], got[k], rtol=1e-5, atol=1e-7, err_msg=k)
