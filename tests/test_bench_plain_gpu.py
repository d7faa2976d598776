"""The benchmark's plain run: the headline leg alone, --steps timed steps, one result line, and
--dump-outputs writing the table the last timed step built (checked here against the C oracle on
the same seeded graph, so the dumped arrays are the ones a caller of the build receives)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIDE_LEGS = ("cpu_baseline", "routing_e2e", "c2_engines", "relay", "c3", "c4", "c5b", "codel", "tbucket",
             "parity_check")


def test_bench_plain_run_is_lean_and_dumps_its_table(tmp_path):
    from oracle import corc
    from shadow_amd import synth
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "node-pairs/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    n = d["config"]["nodes"]
    assert d["value"] == pytest.approx(n * n / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in SIDE_LEGS if k in d]   # those run under --full only

    assert sorted(os.listdir(out)) == ["lat.npy", "loss.npy"]
    lat, loss = np.load(out / "lat.npy"), np.load(out / "loss.npy")
    assert lat.dtype == np.float64 and loss.dtype == np.float32
    assert lat.shape == loss.shape == (n, n)
    assert lat.nbytes + loss.nbytes <= 64 << 20
    el = synth.complete_graph(1000, 1)
    code, olat, oloss, _ = corc.routing(el.n_nodes, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed,
                                        np.arange(el.n_nodes, dtype=np.uint32), threads=corc.max_threads())
    assert code == "OK"
    assert int(olat.max()) < 2**53   # float64 holds every latency exactly
    assert np.array_equal(lat, olat.astype(np.float64))
    assert np.array_equal(loss.view(np.uint32), oloss.view(np.uint32))
