"""An ogbg-ppa gcn / gcn-virtual checkpoint through the exporter and the loaders, no GPU (flowgnn.h: flowgnn_set_model_edge_linear;
DESIGN.md section 4.32): state_dict -> export_weights -> the files -> tests/gcn_edge_linear_ref.forward must be OGB's ppa formulas on that
dict.  The files are float32 and the source float64: the comparison is tests/test_gcn_wide_cpu.py's (rtol 1e-4, atol 2e-5), and the
encoder's file must hold exactly the dict's tensors cast, where the loader and the engine expect them."""
import os

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import gcn_edge_linear_ref as R, gcn_wide_ref as W, gcn_wide_vn_ref as V, gin_edge_linear_ref as GR
from tests.test_export import _bn

L, D, F = 5, 300, 7


def ppa_state_dict(vn, seed):
    """tests/gcn_wide_ref.state_dict / gcn_wide_vn_ref.vn_state_dict (BatchNorms with non-trivial statistics) with ppa's node and edge encoders"""
    rng = np.random.default_rng(seed)
    sd = V.vn_state_dict(seed=seed, vn_w1_scale=1.0 / 16) if vn else W.state_dict(seed=seed)
    sd = {k: v for k, v in sd.items() if "atom_encoder" not in k and "bond_encoder" not in k}
    sd["gnn_node.node_encoder.weight"] = 0.5 * rng.standard_normal((1, D))
    for l in range(L):
        sd[f"gnn_node.convs.{l}.edge_encoder.weight"] = rng.uniform(-1, 1, (D, F)) / np.sqrt(F)
        sd[f"gnn_node.convs.{l}.edge_encoder.bias"] = rng.uniform(-1, 1, D) / np.sqrt(F)
    return sd


def ppa_forward(sd, batch, ef, vn):
    """OGB's ppa GNN (examples/graphproppred/ppa/conv.py: gcn / gcn-virtual, JK='last', no residual, mean pooling) in eval mode, float64,
    nothing folded"""
    row, col = batch.global_edges().T
    N, G = batch.total_nodes, batch.num_graphs
    off, gid = batch.node_offsets(), np.repeat(np.arange(G), batch.nums_of_nodes)
    h = np.tile(sd["gnn_node.node_encoder.weight"], (N, 1))  # node_encoder(x), x all zeros
    vec = np.tile(sd[export.VN_KEY].reshape(1, D), (G, 1)) if vn else np.zeros((G, D))
    deg = np.bincount(row, minlength=N) + 1.0
    norm = deg[row] ** -0.5 * deg[col] ** -0.5
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        h = h + vec[gid]
        x = h @ sd[f"{c}.linear.weight"].T + sd[f"{c}.linear.bias"]
        e = ef.astype(np.float64) @ sd[f"{c}.edge_encoder.weight"].T + sd[f"{c}.edge_encoder.bias"]
        z = np.zeros((N, D))
        np.add.at(z, col, norm[:, None] * np.maximum(x[row] + e, 0.0))
        z = _bn(sd, f"gnn_node.batch_norms.{l}", z + np.maximum(x + sd[f"{c}.root_emb.weight"], 0.0) / deg[:, None])
        if vn and l < L - 1:
            m = f"gnn_node.mlp_virtualnode_list.{l}"
            t = (np.add.reduceat(h, off[:-1], axis=0) + vec) @ sd[f"{m}.0.weight"].T + sd[f"{m}.0.bias"]
            t = np.maximum(_bn(sd, f"{m}.1", t), 0.0) @ sd[f"{m}.3.weight"].T + sd[f"{m}.3.bias"]
            vec = np.maximum(_bn(sd, f"{m}.4", t), 0.0)
        h = z if l == L - 1 else np.maximum(z, 0.0)
    pooled = np.add.reduceat(h, off[:-1], axis=0) / batch.nums_of_nodes[:, None]
    return (pooled @ sd["graph_pred_linear.weight"].T + sd["graph_pred_linear.bias"])[:, 0]


@pytest.mark.parametrize("vn", [False, True], ids=["gcn", "gcn-virtual"])
def test_ppa_checkpoint_through_the_files(vn, tmp_path):
    sd = ppa_state_dict(vn, seed=5 + vn)
    mol = gp.synth_molhiv_batch(6, seed=2)  # (both directions of every edge: OGB's deg^-1/2 and the engine's dinv agree, gcn_wide_ref.ogb_forward)
    batch = gp.GraphBatch(mol.nums_of_nodes, mol.nums_of_edges, np.zeros_like(mol.node_feature), mol.edge_list, mol.edge_attr)  # ppa's x
    ef = GR.features(batch.total_edges, F, 9)
    want = ppa_forward(sd, batch, ef, vn)

    export.export_weights("GCN", sd, str(tmp_path), emb_dim=D, **(dict(virtual_node=True, virtual_node_dim=D) if vn else {}))
    w = weights.load_gcn_weights(str(tmp_path), emb_dim=D)
    el = weights.load_edge_linear(str(tmp_path), emb_dim=D, num_layers=L, model="GCN")
    vnt = weights.load_gcn_virtual_node(str(tmp_path), emb_dim=D) if vn else None
    nemb = w["node_embedding_weight"]
    assert np.array_equal(nemb[0], sd["gnn_node.node_encoder.weight"][0].astype(np.float32)) and not nemb[1:].any()
    assert not w["edge_embedding_weight"].any()
    for l in range(L):
        assert np.array_equal(el["w"][l], sd[f"gnn_node.convs.{l}.edge_encoder.weight"].astype(np.float32))
        assert np.array_equal(el["b"][l], sd[f"gnn_node.convs.{l}.edge_encoder.bias"].astype(np.float32))
    raw = np.fromfile(os.path.join(str(tmp_path), "gcn_ep1_edgelin_dim300.bin"), "<f4")
    assert np.array_equal(raw, np.concatenate([el["w"].ravel(), el["b"].ravel()]))
    assert not os.path.exists(os.path.join(str(tmp_path), weights.edge_linear_file(D)))  # GIN's name is GIN's

    got = R.forward(batch, w, el, ef, vn=vnt).logits
    assert np.allclose(got, want, rtol=1e-4, atol=2e-5), np.abs(got - want).max()  # float32 files vs float64 source


@pytest.mark.parametrize("floats", [L * D * 12, 4 * D * 8], ids=["F = 11", "another depth"])
def test_file_of_no_edge_dim_or_another_depth_is_refused(floats, tmp_path):
    np.zeros(floats, "<f4").tofile(os.path.join(str(tmp_path), weights.edge_linear_file(D, "GCN")))
    with pytest.raises(ValueError, match="1 .. 10"):
        weights.load_edge_linear(str(tmp_path), emb_dim=D, num_layers=L, model="GCN")
