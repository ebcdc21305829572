"""The LDS-DMA ordering rule on the assembly of PNA's single-product translation units (scripts/dev/dma_lint.py; pna_f16.hip,
pna_emb_f16.hip, pna_rows_f16.hip).

The rule itself, as tests/test_dma_lint.py states it: every request meets a covering wait on every path, a counted wait vmcnt(M)
keeps at least M younger loads behind the request (K >= M), and no request is carried across a barrier.  The kernels are pna.hip's,
compiled with half the chunk: they keep its schedule -- the resident kernel's one counted wait, and the next tile's rows that the
per-layer kernel leaves in flight where its loop ends -- so beyond the rule each kernel is held to the figures of its default
counterpart, compiled here beside it: the same counted waits, nothing carried, the same requests in flight at the end, and fewer
requests (15 chunk pieces over 16 waves are one request per wave, not two).  No snapshot.  Needs hipcc, no GPU."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
HIPCC = "/opt/rocm/bin/hipcc"
# translation unit -> {its kernel: (the default translation unit, the default kernel)}
UNITS = {
    "pna_f16": {"pna_resident_f16_kernel": ("pna", "pna_resident_kernel"), "pna_layer_fused_f16_kernel": ("pna", "pna_layer_fused_kernel"),
                "pna_dense_split_f16_kernel": ("pna", "pna_dense_split_kernel")},
    "pna_emb_f16": {"pna_resident_emb_f16_kernel": ("pna_emb", "pna_resident_emb_kernel")},
    "pna_rows_f16": {"pna_resident_rows_f16_kernel": ("pna_rows", "pna_resident_rows_kernel")},
}


def _one(got, name):
    hits = [r for k, r in got.items() if str(len(name)) + name in k]  # (the mangled name: <length>name)
    assert len(hits) == 1, (name, sorted(got))
    return hits[0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_lds_dma_request_is_covered_as_in_the_default_kernels(tmp_path):
    import dma_lint
    files = sorted(set(UNITS) | {d for ks in UNITS.values() for d, _ in ks.values()})

    def asm(f):
        out = str(tmp_path / (f + ".s"))
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "flowgnn_amd", "csrc", f + ".hip"), "-o", out], check=True, capture_output=True)
        return f, dma_lint.snapshot(out)

    with ThreadPoolExecutor(len(files)) as ex:
        got = dict(ex.map(asm, files))
    for unit, kernels in UNITS.items():
        for name, (dunit, dname) in kernels.items():
            r, d = _one(got[unit], name), _one(got[dunit], dname)
            print(unit, name, r, "| default:", d)
            assert r["requests"] > 0 and r["covers_vmcnt0"] + len(r["counted"]) > 0, (name, r)
            assert all(K >= M for M, K in r["counted"]), (name, r)
            assert not r["carried"], (name, r)
            assert [tuple(c) for c in r["counted"]] == [tuple(c) for c in d["counted"]], (name, r, d)
            assert r["in_flight_at_end"] == d["in_flight_at_end"] and not d["carried"], (name, r, d)
            assert r["requests"] < d["requests"], (name, r, d)
