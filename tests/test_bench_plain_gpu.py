"""A plain `bench.py` run (no --full) on the GPU, at a small size: it times exactly --steps steps,
runs none of the side legs, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("cpu_baseline", "claims_tick", "small_flush", "sync_leg", "wire_leg", "pcie_inclusive", "host_tick",
             "cfg4_strong", "cfg5_strips", "host_to_host_tick")


def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--entities", "20000", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["full"] is False and line["steps"] == 7 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["unit"] == "entity-moves/s" and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(20000 / (line["ms_per_step"] * 1e-3), rel=1e-6)
    assert all(line[k] is None for k in SIDE_LEGS) and line["stages_ms_per_tick"] == {}
    assert line["debug_counters"]["flushes"] == 1 + 2 + 7  # populate, warmup, then --steps timed flushes
    counts = np.load(out / "event_counts.npy")
    ent, lev = np.load(out / "enter_pairs.npy"), np.load(out / "leave_pairs.npy")
    assert counts.dtype == ent.dtype == lev.dtype == np.float64
    assert counts.shape == (7, 2) and counts.sum() / 7 == pytest.approx(line["events_per_tick"])
    assert ent.shape == (counts[-1, 0], 2) and lev.shape == (counts[-1, 1], 2) and len(ent) + len(lev) > 0
    for p in (ent, lev):  # directed events of a symmetric relation: (a, b) with (b, a), sorted, slots in range
        assert p.min() >= 0 and p.max() < 20000 and np.all(p[:, 0] != p[:, 1])
        key = p[:, 0] * 2 ** 32 + p[:, 1]
        assert np.all(np.diff(key) > 0)
        assert np.array_equal(np.sort(p[:, 1] * 2 ** 32 + p[:, 0]), key)
    assert not set(map(tuple, ent)) & set(map(tuple, lev))
