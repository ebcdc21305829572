"""A plain `bench.py` run on the GPU: ONE line with the headline figures and nothing that needs a run of its own (those are `--full`),
`--steps` as the number of timed steps, and `--dump-outputs` writing the logits of the last timed step, which are the oracle's logits of
the seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from tests.parity import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"roofline", "aggregation_roofline", "entry_point_host_arrays", "cpu_baseline", "gpu_over_cpu", "parity", "configs"}


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_timed_logits(tmp_path, oracle):
    from flowgnn_amd import weights
    graphs, steps = 300, 3
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--graphs", str(graphs), "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(tmp_path / "out")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == 1, out
    line = json.loads(out[0])
    assert line["unit"] == "graphs/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["finite"] is True
    assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - graphs * 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    assert not FULL_ONLY & set(line), FULL_ONLY & set(line)
    got = np.load(tmp_path / "out" / "logits.npy")
    assert got.dtype == np.float32 and got.shape == (graphs,)
    want = oracle.gin_forward(bench.make_batch("molhiv", graphs, 1234), [weights.synth_gin_weights(seed=7)])
    assert_close(got, want, what="GIN")
