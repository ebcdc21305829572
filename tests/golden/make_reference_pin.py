"""Generates tests/golden/reference_pin_<model>.npz for the six models: outputs of the REFERENCE's own kernel sources, compiled
against the stand-in headers of oracle/hls_standin (make -C oracle ref; tests/ref_pin.py calls them) -- not of the oracle.

Each file holds one batch (40 graphs of the model's dataset shape, 24 more with every sixth edge dropped, duplicate edges and self
loops, then the five tiny graphs of ref_pin.tiny_graphs; 16 + 8 + 5 for the hep10k-shaped models; GIN-VN: with the virtual nodes
added), the seeds of the synthetic weight sets, and per weight case the float logits (`f32_*`, the reference's program in fp32) and the
16-bit patterns (`fx_*`, the reference's program in ap_fixed):
    *_synth     weights.SYNTH[model](seed = weight_seeds[0])
    *_trained   the shipped trained set (tests/golden/ref_weights_<model>.npz, key `trained`)
    *_reload    both synthetic sets, reload_weights switching to the second one mid-batch
    *_synth_per_graph (GAT)   one call per graph: every feature offset is 0 (GAT/src/GAT_compute.cc:72 has no effect)
Needs the reference checkout ($FLOWGNN_REFERENCE).  Run from the repo root:  python tests/golden/make_reference_pin.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from flowgnn_amd import graphpack as gp, weights  # noqa: E402
from tests import ref_pin as rp  # noqa: E402
from tests.golden import make_ref_weights  # noqa: E402

WEIGHT_SEEDS = (7, 8)
SIZES = {"PNA": (16, 8), "DGN": (16, 8)}


def path(model):
    return os.path.join(HERE, f"reference_pin_{model.lower().replace('-', '_')}.npz")


def fixture_batch(model):
    plain, rough = SIZES.get(model, (40, 24))
    base = model.replace("-VN", "")
    eigen = model == "DGN"
    b = gp.concat_batches([rp.dataset_batch(base, plain, 20241019),
                           rp.with_duplicates(rp.directed_variant(rp.dataset_batch(base, rough, 20241020)), 5),
                           rp.tiny_graphs(9, eigen)])
    if not eigen:
        b.node_eigen = None
    return gp.add_virtual_nodes(b) if model == "GIN-VN" else b


def reload_flags(num_graphs):
    rw = np.zeros(num_graphs, np.int32)
    rw[0] = rw[num_graphs // 3] = 1
    return rw


def weight_cases(model, num_graphs):
    """name -> (weight sets, reload_weights or None)"""
    sets = [weights.SYNTH[model](seed=s) for s in WEIGHT_SEEDS]
    return {"synth": (sets[:1], None), "trained": ([make_ref_weights.load(model)], None), "reload": (sets, reload_flags(num_graphs))}


def from_npz(z):
    return gp.GraphBatch(z["nums_of_nodes"], z["nums_of_edges"], z["node_feature"], z["edge_list"], z["edge_attr"],
                         z["node_eigen"] if "node_eigen" in z.files else None)


def reference_outputs(model, b):
    out = {}
    for name, (sets, rw) in weight_cases(model, b.num_graphs).items():
        for form in rp.FORMS:
            out[f"{form}_{name}"] = rp.run(model, form, b, sets, rw)
    if model == "GAT":
        for form in rp.FORMS:
            out[f"{form}_synth_per_graph"] = rp.run_per_graph(model, form, b, weights.SYNTH[model](seed=WEIGHT_SEEDS[0]))
    return out


if __name__ == "__main__":
    assert rp.available(), "no reference checkout and no built oracle/_ref"
    for model in rp.MODELS:
        b = fixture_batch(model)
        fields = dict(nums_of_nodes=b.nums_of_nodes, nums_of_edges=b.nums_of_edges, node_feature=b.node_feature, edge_list=b.edge_list,
                      edge_attr=b.edge_attr, weight_seeds=np.asarray(WEIGHT_SEEDS, np.int32), reload_weights=reload_flags(b.num_graphs))
        if b.node_eigen is not None:
            fields["node_eigen"] = b.node_eigen
        fields.update(reference_outputs(model, b))
        np.savez_compressed(path(model), **fields)
        print("wrote", os.path.basename(path(model)), os.path.getsize(path(model)), "bytes,", b.num_graphs, "graphs", fields["f32_synth"][:3], fields["fx_synth"][:3])
