"""bench.py --dump-outputs end to end on the GPU: the files hold the last timed step, taken before anything --full runs after
the timed region, and two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_REPLAY_ONLY = ["--full", "--no-cpu-baseline", "--no-eer", "--no-extra", "--no-roofline", "--no-fp32-leg", "--no-f16-window"]


def run_bench(out, extra=()):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", out] + list(extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_dump_outputs_are_the_last_timed_step_and_reproducible(tmp_path):
    a = run_bench(str(tmp_path / "a"))
    b = run_bench(str(tmp_path / "b"))
    c = run_bench(str(tmp_path / "c"), FULL_REPLAY_ONLY)      # the re-pack proof replays once more after the dump
    assert c["graph_replay_repacks_weights"] is True and a["graph_replay_repacks_weights"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bn_running_stats.npy", "gradients.npy", "logits.npy", "loss.npy", "parameters.npy", "rank.npy"]
    for n in names:
        x = np.load(tmp_path / "a" / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        for d in "bc":
            np.testing.assert_array_equal(x, np.load(tmp_path / d / n), err_msg="%s differs in run %s" % (n, d))
    assert round(float(np.load(tmp_path / "a" / "loss.npy")[0]), 4) == a["final_loss"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
