"""An ogbg-ppa checkpoint through the exporter and the loader, no GPU (flowgnn.h: flowgnn_set_edge_linear):
state_dict -> export_weights -> the files -> tests/gin_edge_linear_ref.forward must be OGB's ppa formulas on that dict.  The files are
float32, so the claim has two halves: the exporter's tensors before their cast give the direct evaluation to float64 round-off, and
the files hold exactly those tensors cast, where the loader and the engine expect them."""
import os

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import gin_edge_linear_ref as R, gin_wide_ref as W
from tests.test_export import _bn

L, D = 5, 300


def ppa_state_dict(F, seed):
    """tests/gin_wide_ref.state_dict (both BatchNorms with non-trivial statistics, a trained eps) with ppa's node and edge encoders"""
    rng = np.random.default_rng(seed)
    sd = {k: v for k, v in W.state_dict(seed=seed).items() if "atom_encoder" not in k and "bond_encoder" not in k}
    sd["gnn_node.node_encoder.weight"] = 0.5 * rng.standard_normal((1, D))
    for l in range(L):
        sd[f"gnn_node.convs.{l}.edge_encoder.weight"] = rng.uniform(-1, 1, (D, F)) / np.sqrt(F)
        sd[f"gnn_node.convs.{l}.edge_encoder.bias"] = rng.uniform(-1, 1, D) / np.sqrt(F)
    return sd


def ppa_forward(sd, batch, ef):
    """OGB's ppa GNN (examples/graphproppred/ppa/conv.py: gin, JK='last', no residual, mean pooling) in eval mode, float64, nothing folded"""
    row, col = batch.global_edges().T
    h = np.tile(sd["gnn_node.node_encoder.weight"], (batch.total_nodes, 1))  # node_encoder(x), x all zeros
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        e = ef.astype(np.float64) @ sd[f"{c}.edge_encoder.weight"].T + sd[f"{c}.edge_encoder.bias"]
        agg = np.zeros_like(h)
        np.add.at(agg, col, np.maximum(h[row] + e, 0.0))
        z = ((1.0 + sd[f"{c}.eps"][0]) * h + agg) @ sd[f"{c}.mlp.0.weight"].T + sd[f"{c}.mlp.0.bias"]
        z = np.maximum(_bn(sd, f"{c}.mlp.1", z), 0.0) @ sd[f"{c}.mlp.3.weight"].T + sd[f"{c}.mlp.3.bias"]
        z = _bn(sd, f"gnn_node.batch_norms.{l}", z)
        h = z if l == L - 1 else np.maximum(z, 0.0)
    pooled = np.add.reduceat(h, batch.node_offsets()[:-1], axis=0) / batch.nums_of_nodes[:, None]
    return (pooled @ sd["graph_pred_linear.weight"].T + sd["graph_pred_linear.bias"])[:, 0]


@pytest.mark.parametrize("F", [1, 7])
def test_ppa_checkpoint_through_the_files(F, tmp_path):
    sd = ppa_state_dict(F, seed=3 + F)
    mol = gp.synth_molhiv_batch(6, seed=2)
    batch = gp.GraphBatch(mol.nums_of_nodes, mol.nums_of_edges, np.zeros_like(mol.node_feature), mol.edge_list, mol.edge_attr)  # ppa's x
    ef = R.features(batch.total_edges, F, 9)
    want = ppa_forward(sd, batch, ef)

    # the exporter's tensors before the float32 cast: the forward on them is OGB's, to float64 round-off (the folds reorder products)
    w64, eps = W.exported_unrounded(export._ppa_as_molecular(sd, L))
    el64 = {"w": np.stack([sd[f"gnn_node.convs.{l}.edge_encoder.weight"] for l in range(L)]),
            "b": np.stack([sd[f"gnn_node.convs.{l}.edge_encoder.bias"] for l in range(L)])}
    got64 = R.forward(batch, w64, el64, ef, eps=eps, eps_f64=True).logits
    assert np.abs(got64 - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), np.abs(got64 - want).max()

    # the files: exactly those tensors cast, where the loader and the engine expect them
    export.export_weights("GIN", sd, str(tmp_path), keep_eps=True)
    w = weights.load_gin_weights(str(tmp_path), emb_dim=D)
    el = weights.load_edge_linear(str(tmp_path), emb_dim=D, num_layers=L)
    for k in w:
        assert np.array_equal(w[k], np.asarray(w64[k], np.float32).reshape(w[k].shape)), k
    nemb = w["node_embedding_weight"]
    assert np.array_equal(nemb[0], sd["gnn_node.node_encoder.weight"][0].astype(np.float32)) and not nemb[1:].any()
    assert not w["edge_embedding_weight"].any()
    assert el["w"].shape == (L, D, F) and np.array_equal(el["w"], el64["w"].astype(np.float32)) and np.array_equal(el["b"], el64["b"].astype(np.float32))
    raw = np.fromfile(os.path.join(str(tmp_path), "gin_ep1_edgelin_dim300.bin"), "<f4")
    assert np.array_equal(raw, np.concatenate([el["w"].ravel(), el["b"].ravel()]))


def test_file_of_no_edge_dim_is_refused(tmp_path):
    np.zeros(L * D * 12, "<f4").tofile(os.path.join(str(tmp_path), weights.edge_linear_file(D)))  # F would be 11
    with pytest.raises(ValueError, match="1 .. 10"):
        weights.load_edge_linear(str(tmp_path), emb_dim=D, num_layers=L)
