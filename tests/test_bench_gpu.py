"""bench.py as it is run for every change: a plain run (no --full) prints one short line for the headline alone, and --dump-outputs writes
what its last timed step computed -- the same bits from two runs with the same arguments, other bits after one more step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("position", "velocity", "render_color", "render_data", "slot")


def _plain_run(out_dir, steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "0", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, "stdout carries the result line alone"
    return json.loads(lines[0])


def test_a_plain_run_times_exactly_its_steps_and_dumps_the_last_ones_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _plain_run(a, 3)
    assert d["metric"].startswith("Mparticle-steps/sec") and d["unit"] == "Mparticle-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["timed_blocks"]["blocks"] == 1 and d["timed_blocks"]["steps_per_block"] == 3 and d["timed_blocks"]["headline"] == "the one block"
    assert d["config"]["particles_per_gpu"] == 64 * 1024 * 1024 and d["config"]["workload"].startswith("cfg4-64M on one GPU")
    assert d["ms_per_step"] > 0 and abs(d["value"] - 64 * 1024 * 1024 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    for k in ("lighting", "cpu_baseline", "next_rows", "cfg4_share_8m_particles", "hbm_calibration"):
        assert k not in d, "%s belongs to --full" % k
    assert len(json.dumps(d)) < 4096
    total = 0
    for name in NAMES:
        x = np.load(os.path.join(a, "particles_%s.npy" % name))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        total += x.nbytes
    assert total <= 64 << 20
    pos = np.load(os.path.join(a, "particles_position.npy"))
    assert (pos[:, 3] > 0).all(), "nobody dies in the headline's steps (life in w)"
    _plain_run(b, 3)
    for name in NAMES:
        assert np.array_equal(np.load(os.path.join(a, "particles_%s.npy" % name)), np.load(os.path.join(b, "particles_%s.npy" % name))), name
    # the dump is the state after the LAST timed step: one step more moves every sampled particle (same slots, same life decay per step)
    c = str(tmp_path / "c")
    assert _plain_run(c, 4)["steps"] == 4
    assert np.array_equal(np.load(os.path.join(a, "particles_slot.npy")), np.load(os.path.join(c, "particles_slot.npy")))
    p3, p4 = np.load(os.path.join(a, "particles_position.npy")), np.load(os.path.join(c, "particles_position.npy"))
    assert (p4[:, 3] < p3[:, 3]).all(), "life decays once more in the fourth step"
    assert (p4[:, :3] != p3[:, :3]).any(axis=1).mean() > 0.99, "the fourth step moves the particles"
