"""Host-side pieces of bench.py that need no GPU: the CPU count the cpu_baseline leg is sized from, the model table, the writer of
--dump-outputs and the checks of the command line."""
import builtins
import io
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_open(files):
    real = builtins.open

    def opener(path, *a, **k):
        if path in files:
            if files[path] is None:
                raise OSError(path)
            return io.StringIO(files[path])
        return real(path, *a, **k)
    return opener


def test_effective_cpus_follows_the_cgroup_quota(monkeypatch):
    monkeypatch.setattr(bench.os, "sched_getaffinity", lambda pid: set(range(256)), raising=False)
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": "1600000 100000\n"}))
    assert bench.effective_cpus() == 16  # the GPU pool's boxes: 256 hardware threads under a 16-CPU quota
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": "max 100000\n"}))
    assert bench.effective_cpus() == 256
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": "150000 100000\n"}))
    assert bench.effective_cpus() == 2  # a fractional quota rounds up
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": None,
                                                      "/sys/fs/cgroup/cpu/cpu.cfs_quota_us": "800000\n",
                                                      "/sys/fs/cgroup/cpu/cpu.cfs_period_us": "100000\n"}))
    assert bench.effective_cpus() == 8  # cgroup v1
    monkeypatch.setattr(builtins, "open", _fake_open({"/sys/fs/cgroup/cpu.max": None, "/sys/fs/cgroup/cpu/cpu.cfs_quota_us": None}))
    assert bench.effective_cpus() == 256


def test_model_table_is_complete():
    for name, m in bench.MODELS.items():
        assert {"metric", "dataset", "graphs", "agg_bytes", "flops", "hbm_kernels", "mfma_kernels", "workload"} <= set(m), name
        n, e = 1000, 2200
        assert m["agg_bytes"](n, e) > 0 and m["flops"](n, e) > 0
        fb = m.get("fused_bytes")
        if isinstance(fb, dict):
            assert set(fb) <= set(m["mfma_kernels"])
            assert all(f(n, e) > 0 for f in fb.values())
        elif fb is not None:
            assert fb(n, e) > 0


def test_dump_outputs_writes_float32_and_samples_past_the_limit(tmp_path, monkeypatch):
    a = np.arange(1000, dtype=np.float64).reshape(500, 2) * 0.5
    bench.dump_outputs(str(tmp_path / "all"), {"h": a})
    got = np.load(tmp_path / "all" / "h.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    assert not (tmp_path / "all" / "h_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1600)  # 16 B per row (two floats + an 8-byte row number): 100 rows
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"h": a})
    idx = np.load(tmp_path / "s1" / "h_index.npy")
    got = np.load(tmp_path / "s1" / "h.npy")
    assert idx.dtype == np.float64 and len(idx) == 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(got, a[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "h_index.npy"))  # a fixed sample: the same rows in every run


def test_full_only_options_and_step_counts_are_checked_before_any_work():
    for args, msg in ((["--configs", "on"], "--full"), (["--inject-parity-failure"], "--full"), (["--steps", "0"], "--steps")):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and msg in p.stderr, (args, p.returncode, p.stderr[-500:])
        assert p.stdout == ""
