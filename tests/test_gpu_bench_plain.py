"""A plain bench.py run: the headline line alone, --steps timed steps, and
--dump-outputs writing the trained state of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

pytestmark = pytest.mark.gpu

# params / targets arenas of the Humanoid 2x256 SAC trainer hold at least the
# unpadded parameter counts (policy 171,043 + two critics 333,826; two targets)
N_PARAMS, N_TARGETS = 171_043 + 333_826, 333_826


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "6", "--warmup", "3",
                        "--replay", "20000", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 6 and out["warmup"] == 3 and out["n_gpus"] == 1
    assert out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (both rounded in the line)
    assert out["value"] * out["ms_per_step"] == pytest.approx(1e3, rel=1e-2)
    # the legs that take runs of their own are --full's
    for k in ("roofline", "kernels", "b4096", "cpu_baseline", "dp1", "exploration", "goac"):
        assert k not in out, k
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert {"params", "targets", "grads", "adam_m", "adam_v", "alpha_state"} <= set(got)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["params"].size >= N_PARAMS and got["targets"].size >= N_TARGETS
    assert got["params"].shape == got["grads"].shape == got["adam_m"].shape == got["adam_v"].shape
    # nine steps were taken: the gradients and both Adam moments are populated
    assert np.abs(got["grads"]).max() > 0 and np.abs(got["adam_m"]).max() > 0
    assert got["adam_v"].min() >= 0 and got["adam_v"].max() > 0
