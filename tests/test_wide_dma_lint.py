"""The LDS-DMA ordering rule on the assembly of the three files of width 300 -- gcn_wide.hip, gin_wide.hip and wide_attn.hip
(scripts/dev/dma_lint.py; DESIGN.md sections 4.16 to 4.21): every kernel of a file that issues LDS-DMA -- the layer kernels, their
virtual-node instances by name, the final kernel, the update kernel and the attention gate -- has every request covered by an
`s_waitcnt vmcnt(0)` on every control-flow path, and none by a counted wait (vmcnt(M), M > 0), which would hold only while the
compiler keeps M younger loads behind the request.  The rule alone: no snapshot.  Needs hipcc, no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
HIPCC = "/opt/rocm/bin/hipcc"

KERNELS = {
    "gcn_wide": ("gcw_layer_kernel", "gcw_layer_vn_kernel", "gcw_final_kernel"),
    "gin_wide": ("gw_layer_kernel", "gw_layer_vn_kernel", "gw_vn_update_kernel"),
    "wide_attn": ("attn_gate_kernel",),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("unit", sorted(KERNELS))
def test_every_lds_dma_request_is_covered_by_a_full_wait(unit, tmp_path):
    import dma_lint
    out = str(tmp_path / (unit + ".s"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "flowgnn_amd", "csrc", unit + ".hip"), "-o", out], check=True, capture_output=True)
    got = dma_lint.snapshot(out)
    for want in KERNELS[unit]:
        assert sum(want + "I" in k for k in got) == 1, (want, sorted(got))  # (the mangled name: <length>name I <template arguments>)
    for k, r in got.items():
        print(k, r)
        assert r["requests"] > 0 and r["covers_vmcnt0"] == r["requests"], (k, r)
        assert not r["counted"] and not r["carried"] and r["in_flight_at_end"] == 0, (k, r)
