"""The LDS-DMA ordering rule on the assembly of gcn_wide_f16.hip (scripts/dev/dma_lint.py), with the assertions
of tests/test_wide_f16_dma_lint.py: the four layer kernels of GCN's f16 mode at width 300 -- plain, virtual node, and each with OGB's
residual and JK sum -- have every request covered by an `s_waitcnt vmcnt(0)` on every control-flow path, none by a counted wait, none
carried across a barrier and none in flight at the end (the odd step count leaves one step behind the loop: it requests nothing).
The rule alone: no snapshot.  Needs hipcc, no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("gcw_layer_f16_kernel", "gcw_layer_vn_f16_kernel", "gcw_layer_jk_f16_kernel", "gcw_layer_vn_jk_f16_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_lds_dma_request_is_covered_by_a_full_wait(tmp_path):
    import dma_lint
    out = str(tmp_path / "gcn_wide_f16.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "flowgnn_amd", "csrc", "gcn_wide_f16.hip"), "-o", out], check=True, capture_output=True)
    got = dma_lint.snapshot(out)
    assert len(got) == len(KERNELS), sorted(got)
    for want in KERNELS:
        assert sum(want + "I" in k for k in got) == 1, (want, sorted(got))  # (the mangled name: <length>name I <template arguments>)
    for k, r in got.items():
        print(k, r)
        assert r["requests"] > 0 and r["covers_vmcnt0"] == r["requests"], (k, r)
        assert not r["counted"] and not r["carried"] and r["in_flight_at_end"] == 0, (k, r)
