"""bench.py's plain run: it times exactly --steps steps, leaves what only --full measures out of its line, and --dump-outputs writes what
the last timed step computed -- the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(d):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "cfg1",
           "--dump-outputs", str(d)]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(d / f) for f in os.listdir(d)}


@pytest.mark.timeout(700)
def test_bench_plain_run_dumps_the_last_step(tmp_path):
    r, a = _bench_dump(tmp_path / "a")
    assert r["steps"] == 3 and r["warmup"] == 1 and r["dtype"] == "f32" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0 and abs(r["value"] - 2 * 256 * 256 / (r["ms_per_step"] * 1e-3)) < 1e-3 * r["value"]
    assert not {"roofline", "step_roofline", "fwd_only", "cpu_baseline"} & set(r)

    assert set(a) == {"loss", "prob", "logits", "params", "grads", "buffers"}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["loss"].shape == () and a["logits"].shape == a["prob"].shape == (2, 1, 256, 256)
    np.testing.assert_allclose(a["prob"], 1 / (1 + np.exp(-a["logits"].astype(np.float64))), rtol=0, atol=1e-5)
    # Unet(1,1,32) has 7.8M parameters: a seeded sample of 2^21 of them, and of their gradients
    assert a["params"].shape == a["grads"].shape == (1 << 21,) and np.abs(a["grads"]).max() > 0

    # a second run computes the same: the forward to rounding, gradients to the order of the float atomics of the weight gradients, the
    # parameters after Adam to a small fraction of one lr = 1e-3 step (steps that trained on from each other drift by many)
    _, b = _bench_dump(tmp_path / "b")
    for k in ("loss", "prob", "logits", "buffers"):
        np.testing.assert_allclose(b[k], a[k], rtol=0, atol=1e-6 * float(np.abs(a[k]).max()), err_msg=k)
    np.testing.assert_allclose(b["grads"], a["grads"], rtol=0, atol=1e-5 * float(np.abs(a["grads"]).max()), err_msg="grads")
    np.testing.assert_allclose(b["params"], a["params"], rtol=0, atol=1e-4, err_msg="params")
