"""Shape sweeps and seeded random batches on every width-300 kernel instance: gin, gin-virtual, gcn and
gcn-virtual under each (JK, residual) setting, and gin's eight again in f16 mode -- 24 instances, one engine each, through the route a
user takes (state_dict -> export_weights -> files -> Engine.load_weights_dir -> flags -> kernels).

Cases (tests/wide_cases.py): the fixed families the default instances already pass -- (a) paths and (b) isolated nodes at every row
tile's edge, (c) one-node graphs around a hub and a long path whose sources lie in another workgroup's 128-row tile, (e) 1 / 15 / 16 /
17 / 33 graphs around the update's 16-graph column tile (virtual-node rows), (f) 128 k + 1, 128 k + 127 and 128 k nodes -- and three
seeded random batches, each also run as two shards cut at a seeded graph index.

Expected values: the float64 forward of tests/ogb_jk_torch.py / tests/ogb_gcn_jk_torch.py on the exported files (f16=True for the
f16 rows).  Tolerance: the project's rule and nothing else, |gpu - want| <= 1e-4 (scale + |want|), scale = the forward's largest
activation (tests/parity.py), on logits, graph embeddings, node embeddings (= r) and h_5; in f16 mode the f16 rule, 2e-4, on the
logits, the rows printed with their ratio and not asserted (as section 4.22 does).  Every comparison prints err_ratio.
tests/test_wide_shapes_cpu.py asserts on the references alone what is relied on here: every case stays below half the range
threshold (so exact_reruns() does not move and the kernels under test compute the answer), and the residual or the JK store left out
for the LAST NODE only, or for COLUMNS 288 .. 299 only, misses the rule by at least 10 x on every fixed family (smallest 50.6) -- so a
`node < n_tot - 1` or `col < 288` guard on either stream turns this file red.

What ran: the fast layer slot (gin_wide_layer, gin_wide_layer_f16, gcn_wide_layer), not its _f32 form, and no width-100 kernel.
Shards: the concatenation within the same rule; for gin in the default mode bit for bit the unsplit run's (what
tests/test_jk_residual_gpu.py's placement test promises), for GCN within the bound only (section 4.19).
Readouts: sum and max pooling, the attention and the set2set readout (2 steps) on (a) and one random batch, on the (sum, residual)
instances of gin and gcn without the virtual node (section 4.24 says why not with it).

Findings: no instance missed its bound.  Worst err_ratio per instance over all cases and shards, measured on an MI355X (logits / graph
embeddings / r / h_5; the table of DESIGN.md section 4.26):
  gin-last 0.0004 / 0.0017 / 0.0036 / 0.0036          gin-last-res 0.0006 / 0.0028 / 0.0057 / 0.0057
  gin-sum 0.0006 / 0.0027 / 0.0061 / 0.0038           gin-sum-res 0.0019 / 0.0041 / 0.0074 / 0.0046
  gin-virtual-last 0.0002 / 0.0006 / 0.0008 / 0.0008  gin-virtual-last-res 0.0004 / 0.0015 / 0.0016 / 0.0016
  gin-virtual-sum 0.0005 / 0.0023 / 0.0034 / 0.0008   gin-virtual-sum-res 0.0031 / 0.0052 / 0.0054 / 0.0017
  gcn-last 0.0014 / 0.0077 / 0.0085 / 0.0085          gcn-last-res 0.0013 / 0.0038 / 0.0055 / 0.0055
  gcn-sum 0.0020 / 0.0042 / 0.0067 / 0.0052           gcn-sum-res 0.0021 / 0.0037 / 0.0053 / 0.0019
  gcn-virtual-last 0.0001 / 0.0006 / 0.0015 / 0.0015  gcn-virtual-last-res 0.0004 / 0.0019 / 0.0019 / 0.0019
  gcn-virtual-sum 0.0003 / 0.0017 / 0.0018 / 0.0019   gcn-virtual-sum-res 0.0018 / 0.0037 / 0.0039 / 0.0014
  f16 mode, logits against the f16 rule: gin 0.054 / 0.123 / 0.056 / 0.054 (last, last-res, sum, sum-res), gin-virtual 0.035 / 0.012 /
  0.021 / 0.031; the rows, printed only, up to 1.31.  Readouts: pooling <= 0.0066, attention <= 0.025, set2set <= 0.020.
With gw_layer_body's residual add put under `node < n_tot - 1` and gcw_ext_store's JK store under `col < 288` (tried and reverted), 19
of the 32 ids fail on case (a): every default-mode instance that runs either line, and the f16 and GCN rows that share the update kernel.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import weights  # noqa: E402
from tests import attn_pool_ref as A, set2set_ref as S, wide_cases as C  # noqa: E402
from tests.parity import assert_close, err_ratio  # noqa: E402
from tests.test_embeddings_gpu import launched  # noqa: E402
from tests.test_gcn_wide_gpu import NARROW_SLOTS as GCN_NARROW  # noqa: E402
from tests.test_gin_wide_f16_gpu import F16_REL  # noqa: E402

pytestmark = pytest.mark.gpu
GIN_NARROW = {"gin_resident", "gin_tile_build", "gin_layer_fused", "gin_aggregate", "gin_mlp", "gin_ogb_vn"}
GIN_SLOTS = {"gin_wide_layer", "gin_wide_layer_f16", "gin_wide_layer_f32"}
REL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    if torch.cuda.is_available():
        torch.cuda.init()


engine = C.engine


def check_slots(i, names):
    """The instance's fast layer slot ran; its exact form, the other numeric mode's and every width-100 kernel did not."""
    if i.kind == "gin":
        fast = "gin_wide_layer_f16" if i.f16 else "gin_wide_layer"
        assert names & GIN_SLOTS == {fast} and not names & GIN_NARROW, names
    else:
        assert "gcn_wide_layer" in names and "gcn_wide_layer_f32" not in names and not names & GCN_NARROW, names


def run(e, i, b):
    """One forward -> (logits, pooled, r, h_5), with the slots checked and exact_reruns() where it was."""
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(b, return_embeddings=True, return_node_embeddings=True)))
    logits, pooled, rows = (np.array(x) for x in res["got"])
    h5 = np.array(e.final_h())
    check_slots(i, names)
    assert e.exact_reruns() == before, (e.exact_reruns(), before)
    return logits, pooled, rows.reshape(b.total_nodes, 300), h5.reshape(b.total_nodes, 300)


def compare(i, what, got, ref, worst):
    """The rule on the four outputs (f16 mode: the f16 rule on the logits, the rest printed); worst: name -> largest ratio so far."""
    rel = F16_REL if i.f16 else REL
    for name, g, want in zip(("logits", "pooled", "rows", "h5"), got, (ref.logits, ref.pooled, ref.rows, ref.h5)):
        r = err_ratio(g, want, ref.scale, rel)
        asserted = name == "logits" or not i.f16
        print(C.name_of(i), what, name, f"err_ratio {r:.4f} (scale {ref.scale:.4g}){'' if asserted else ' (printed, not asserted)'}")
        assert g.shape == want.shape, (what, name, g.shape, want.shape)
        if asserted:
            worst[name] = max(worst.get(name, 0.0), r)
            assert_close(g, want, scale=ref.scale, rel=rel, what=(C.name_of(i), what, name))


# ---------------------------------------------------------------- every instance: the fixed families, the random batches, the shards
@pytest.mark.parametrize("instance", C.INSTANCES, ids=C.IDS)
def test_shapes_and_random_batches(instance):
    i, worst = instance, {}
    e = engine(i)
    try:
        for name, b in C.cases_of(i):
            ref = C.cached_reference(i, name)
            got = run(e, i, b)
            compare(i, name, got, ref, worst)
            if not name.startswith("random"):
                continue
            # two shards of the job, cut at a seeded graph index
            cut, off = C.shard_cut(int(name.split("-")[1]), b), b.node_offsets()
            assert 0 < cut < b.num_graphs
            e.set_job_totals(b.total_nodes, b.total_edges)
            parts = [run(e, i, b.slice(lo, hi)) for lo, hi in ((0, cut), (cut, b.num_graphs))]
            e.set_job_totals(-1, -1)
            assert parts[0][2].shape[0] == off[cut]
            joined = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
            compare(i, f"{name}, two shards cut at graph {cut}", joined, ref, worst)
            if i.kind == "gin" and not i.f16:
                for k, what in enumerate(("logits", "pooled", "rows", "h5")):
                    assert joined[k].tobytes() == got[k].tobytes(), (name, cut, what)
        assert e.exact_reruns() == 0
    finally:
        e.close()
    print(C.name_of(i), "worst err_ratio", " ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ---------------------------------------------------------------- the readouts read r at these shapes too
READOUTS = ["sum", "max", "attention", "set2set"]


@pytest.mark.parametrize("readout", READOUTS)
@pytest.mark.parametrize("instance", C.READOUT_INSTANCES, ids=[C.name_of(i) for i in C.READOUT_INSTANCES])
def test_readouts(instance, readout):
    i = instance
    w = C.tensors(i.kind, i.vn, i.jk, i.res)[0]
    e = engine(i, pooling=readout if readout in ("sum", "max") else "mean")
    try:
        if readout == "attention":
            gate = weights.synth_attention_pooling()
            e.set_attention_pooling(gate)
        elif readout == "set2set":
            s2s = weights.synth_set2set()
            e.set_set2set_pooling(s2s, steps=2)
        for name in ("a-paths", f"random-{C.SEEDS[0]}"):
            b = dict(C.cases_of(i))[name]
            what = (C.name_of(i), readout, name)
            before = e.exact_reruns()
            if readout in ("sum", "max"):
                ref = C.cached_reference(i, name, pooling=readout)
                logits, pooled, rows = (np.array(x) for x in e.forward(b, return_embeddings=True, return_node_embeddings=True))
                want_logits, want_pooled, scale = ref.logits, ref.pooled, ref.scale
            elif readout == "attention":
                ref, stats = C.cached_reference(i, name), {}
                want_pooled, want_logits, _ = A.readout(ref.rows, b, gate, w["graph_pred_weights"], w["graph_pred_bias"], stats=stats)
                scale = max(ref.scale, stats["s_max"], stats["hidden_max"])
                logits, pooled, rows = (np.array(x) for x in e.forward(b, return_embeddings=True, return_node_embeddings=True))
            else:
                ref, stats = C.cached_reference(i, name), {}
                _, want_logits, _ = S.readout(ref.rows, b, s2s, steps=2, stats=stats)
                scale = max(ref.scale, stats["q_max"], stats["e_max"], float(np.abs(want_logits).max()))
                logits, rows = (np.array(x) for x in e.forward(b, return_node_embeddings=True))
                pooled = want_pooled = None
            names = launched(e, lambda: e.run())
            check_slots(i, names)
            assert e.exact_reruns() == before
            if readout == "attention":
                assert "attn_gate" in names and "attn_pool_rows" in names, names
            if readout == "set2set":
                assert "s2s_lstm" in names and "s2s_head" in names, names
            pairs = [("rows", rows.reshape(ref.rows.shape), ref.rows), ("logits", logits, want_logits)]
            if pooled is not None:
                pairs.append(("pooled", pooled, want_pooled))
            for out, g, want in pairs:
                print(what, out, f"err_ratio {err_ratio(g, want, scale, REL):.4f} (scale {scale:.4g})")
                assert_close(g, want, scale=scale, rel=REL, what=(what, out))
    finally:
        e.close()
