"""bench.py on the GPU: a plain run prints the headline figure and nothing that --full adds, and both kinds of run time and
dump the very same steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "traced_samples_per_s", "live_fraction", "value_contracted", "parity", "interactive",
             "cpu_baseline", "gpu_over_cpu", "other_configs")


def _run(extra, dump_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(dump_dir)] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_and_full_runs_time_and_dump_the_same_steps(tmp_path):
    plain = _run([], tmp_path / "plain")
    assert plain["metric"] == "Msamples/s (pixels*spp/s)" and plain["unit"] == "Msamples/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["steps"] == 4 and plain["warmup"] == 2 and plain["n_gpus"] == 1
    cfg = plain["config"]
    samples = cfg["width"] * cfg["height"] * cfg["spp_per_step"]
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(samples / plain["ms_per_step"] / 1e3, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in plain]

    full = _run(["--full", "--no-cpu-baseline", "--no-other-configs"], tmp_path / "full")
    assert full["roofline"]["bound"] in ("valu", "l2_miss_fabric") and 0 < full["traced_samples_per_s"] <= full["value"]
    assert full["parity"]["ok"] is True and full["value_contracted"]["value"] > 0
    assert full["config"] == cfg

    # the timed steps render the same samples with or without --full: what they returned is the same, bit for bit
    for name in ("accum", "rgb8"):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (cfg["height"], cfg["width"], 3)
        assert np.array_equal(a, b), name
    assert np.load(tmp_path / "plain" / "accum.npy").max() > 0
