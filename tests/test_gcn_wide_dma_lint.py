"""The LDS-DMA ordering rule on gcn_wide.hip's assembly (scripts/dev/dma_lint.py; DESIGN.md sections 4.18, 4.19): every kernel of the
file that issues LDS-DMA -- the layer kernel, its virtual-node instance by name, and the final kernel -- has every request covered by an
`s_waitcnt vmcnt(0)` on every control-flow path, and none by a counted wait (vmcnt(M), M > 0), which would hold only while the
compiler keeps M younger loads behind the request.  The rule alone: no snapshot.  Needs hipcc, no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_lds_dma_request_of_gcn_wide_is_covered_by_a_full_wait(tmp_path):
    import dma_lint
    out = str(tmp_path / "gcn_wide.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "flowgnn_amd", "csrc", "gcn_wide.hip"), "-o", out], check=True, capture_output=True)
    got = dma_lint.snapshot(out)
    for want in ("gcw_layer_kernel", "gcw_layer_vn_kernel", "gcw_final_kernel"):
        assert sum(want + "I" in k for k in got) == 1, (want, sorted(got))  # (the mangled name: <length>name I <template arguments>)
    for k, r in got.items():
        print(k, r)
        assert r["requests"] > 0 and r["covers_vmcnt0"] == r["requests"], (k, r)
        assert not r["counted"] and not r["carried"] and r["in_flight_at_end"] == 0, (k, r)
