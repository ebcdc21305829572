"""An ogbg-code2 checkpoint through the exporter and the readers, no GPU (flowgnn.h: flowgnn_set_ast_encoder, flowgnn_set_vocab_head;
DESIGN.md section 4.33): tests/code2_torch's model -> export_weights -> the files -> the arrays read back are the state_dict's, and
tests/code2_ref.forward on them is the torch model's forward."""
import os

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import code2_ref as R, code2_torch as T, gin_edge_linear_ref as EL
from tests.parity import assert_close
from tests.wide_cases import isolated, path

D, L, P, V, SIZES = 300, 5, 3, 37, (5, 7, 3)  # tables of a few rows: n_types, n_attrs, max_depth


def test_code2_checkpoint_through_the_files(tmp_path):
    model = T.make_model(V, P, *SIZES, seed=4)
    sd, d = {k: v.numpy() for k, v in model.state_dict().items()}, str(tmp_path)
    with pytest.raises(export.ExportError, match="ogbg-code2"):
        export.export_weights("GCN", sd, d, emb_dim=300)
    assert not os.listdir(d)  # refused before any file is written
    f32 = lambda k: sd[k].astype(np.float32)
    export.export_weights("GIN", sd, d, keep_eps=True)

    ast = weights.load_ast_encoder(d)
    assert [ast[k].shape[0] for k in ("type", "attr", "depth")] == [SIZES[0], SIZES[1], SIZES[2] + 1]
    for k, name in (("type", "type_encoder"), ("attr", "attribute_encoder"), ("depth", "depth_encoder")):
        assert np.array_equal(ast[k], f32(f"gnn_node.node_encoder.{name}.weight")), k
    head = weights.load_vocab_head(d)
    assert head["w"].shape == (P, V, D) and head["b"].shape == (P, V)
    for p in range(P):
        assert np.array_equal(head["w"][p], f32(f"graph_pred_linear_list.{p}.weight")) and np.array_equal(head["b"][p], f32(f"graph_pred_linear_list.{p}.bias"))
    el = weights.load_edge_linear(d, emb_dim=D, num_layers=L)
    assert el["w"].shape == (L, D, 2)  # F = 2, recovered from the file's size
    for l in range(L):
        assert np.array_equal(el["w"][l], f32(f"gnn_node.convs.{l}.edge_encoder.weight")) and np.array_equal(el["b"][l], f32(f"gnn_node.convs.{l}.edge_encoder.bias"))
    eps = weights.load_gin_eps(d, emb_dim=D)
    assert np.array_equal(eps, np.array([sd[f"gnn_node.convs.{l}.eps"][0] for l in range(L)], np.float32)) and eps.all()
    w = weights.load_gin_weights(d, emb_dim=D)
    for k in ("node_embedding_weight", "edge_embedding_weight", "graph_pred_weights", "graph_pred_bias"):
        assert not w[k].any(), k  # what the engine does not read while the encoders are on, and a zero head of the model's own
    # the headers: the counts, as int32, in front of the float32
    assert np.fromfile(os.path.join(d, "gin_ep1_astenc_dim300.bin"), "<i4", 4).tolist() == [D, SIZES[0], SIZES[1], SIZES[2]]
    assert np.fromfile(os.path.join(d, "gin_ep1_vocabhead_dim300.bin"), "<i4", 3).tolist() == [D, P, V]

    # the folded MLPs: the float64 forward on the files' arrays is the torch model's, inside the bound the GPU tests hold the engine to
    batch = gp.concat_batches([path(15, 1), isolated(2, 2), path(17, 3)])
    x, depth = R.ast_nodes(batch.total_nodes, *SIZES, seed=5)
    ef = EL.features(batch.total_edges, 2, 6)
    rows, pooled, logits = T.run(model, batch, x, depth, ef)
    ref = R.forward(batch, w, el, ef, (ast["type"], ast["attr"], ast["depth"]), x, depth, eps=eps)
    assert_close(ref.rows, rows, scale=ref.scale, what="rows")
    assert_close(ref.pooled, pooled, scale=ref.scale, what="pooled")
    assert not np.any(ref.logits)  # the model's own head is the zero one
    R.check_tokens(logits.argmax(axis=2).astype(np.int32), logits.max(axis=2), R.head_logits(pooled, head["w"], head["b"]), what="the files' head on torch's pooled rows")

