"""The LDS-DMA ordering rule on the assembly of DGN's single-product translation units (scripts/dev/dma_lint.py; dgn_f16.hip,
dgn_emb_f16.hip, dgn_rows_f16.hip).

The rule itself, as tests/test_dma_lint.py states it: every request meets a covering wait on every path, a counted wait vmcnt(M)
keeps at least M younger loads behind the request (K >= M), and no request is carried across a barrier that does not order it.  The
kernels are dgn.hip's, compiled with half the chunk: they keep its schedule.  dgn_resident_kernel carries requests across barriers by
design -- a tile's first chunk and the next tile's records across the barrier that follows them, the head block across the barrier
that publishes the rows of h_4; each is waited for (vmcnt(0)) ahead of the barrier that publishes it -- so beyond the rule each kernel
is held to the figures of its default counterpart, compiled here beside it: no counted waits where it has none, nothing in flight at
the end, nothing carried that the default kernel does not carry (as a multiset of the lint's figures per barrier), and fewer requests
(seven chunk pieces over eight waves are one request per wave, not two).  The per-layer matrix-pipe kernel stages its weights with
plain loads: it has no request in either mode.  No snapshot.  Needs hipcc, no GPU."""
import os
import subprocess
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
HIPCC = "/opt/rocm/bin/hipcc"
# translation unit -> {its kernel: (the default translation unit, the default kernel)}
UNITS = {
    "dgn_f16": {"dgn_resident_f16_kernel": ("dgn", "dgn_resident_kernel")},
    "dgn_emb_f16": {"dgn_resident_emb_f16_kernel": ("dgn_emb", "dgn_resident_emb_kernel")},
    "dgn_rows_f16": {"dgn_resident_rows_f16_kernel": ("dgn_rows", "dgn_resident_rows_kernel")},
}


def _all(got, name):
    return [r for k, r in got.items() if str(len(name)) + name in k]  # (the mangled name: <length>name)


def _one(got, name):
    hits = _all(got, name)
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
            assert [tuple(c) for c in r["counted"]] == [tuple(c) for c in d["counted"]], (name, r, d)
            assert r["in_flight_at_end"] == 0 and d["in_flight_at_end"] == 0, (name, r, d)
            assert not (Counter(r["carried"]) - Counter(d["carried"])), (name, r, d)  # nothing carried that the default does not carry
            assert r["requests"] < d["requests"], (name, r, d)
    # the per-layer matrix-pipe kernel's instances issue no request (the lint lists the kernels that do): its weights come by plain loads
    assert not _all(got["dgn_f16"], "dgn_layer_mfma_f16_kernel") and len(got["dgn_f16"]) == 1, sorted(got["dgn_f16"])
