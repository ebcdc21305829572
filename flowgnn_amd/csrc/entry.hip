// entry.hip -- the reference-compatible entry points: <M>_compute_graphs, their _mt forms and flowgnn_entry_*.
#include "engine_internal.h"
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

extern "C" {

// ------------------------------------------------------------------ reference-compatible entry points
// Split the batch into runs of constant weight set (reload_weights semantics of
// GIN/src/GIN_compute.cc:44,51-53) and run each through a process-wide group of engines per model: one engine on device 0
// unless flowgnn_entry_set_devices (or FLOWGNN_DEVICES=0,1,.. at the first call) lists more.
static std::mutex g_entry_mutex;
static flowgnn_group* g_entry_group[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
static std::vector<int> g_entry_devices;  // empty: not decided yet (the environment is asked at the first call)
static int g_entry_pipeline = 0;          // flowgnn_entry_set_pipeline: ranges per engine (0: by the size of the host arrays, 1: off)
static std::vector<std::pair<std::string, double>> g_entry_options[6];
static int g_entry_pooling[6] = {0, 0, 0, 0, 0, 0};  // flowgnn_entry_set_pooling (FLOWGNN_POOL_MEAN)
static bool g_entry_eps_on[6] = {false, false, false, false, false, false};  // flowgnn_entry_set_gin_eps: one vector for every weight set
static float g_entry_eps[6][5] = {};
// The weight set an entry-point group holds, kept on the host: a caller that reloads the SAME set on every graph
// (reload_weights = 1 everywhere is legal in the reference and cheap there) must not pay a repack + upload per graph.
// Compared with memcmp -- no hash, no collision to reason about.
static std::vector<float> g_entry_wcopy[6];
static bool same_weights(int model, int ntens, const float* const* t, const size_t* elems) {
    size_t total = 0;
    for (int i = 0; i < ntens; i++) total += elems[i];
    const std::vector<float>& c = g_entry_wcopy[model];
    if (c.size() != total) return false;
    size_t off = 0;
    for (int i = 0; i < ntens; i++) {
        if (memcmp(c.data() + off, t[i], elems[i] * sizeof(float)) != 0) return false;
        off += elems[i];
    }
    return true;
}
static void remember_weights(int model, int ntens, const float* const* t, const size_t* elems) {
    std::vector<float>& c = g_entry_wcopy[model];
    c.clear();
    for (int i = 0; i < ntens; i++) c.insert(c.end(), t[i], t[i] + elems[i]);
}

static void entry_drop_groups() {
    for (int m = 0; m < 6; m++) {
        if (g_entry_group[m]) flowgnn_group_destroy(g_entry_group[m]);
        g_entry_group[m] = nullptr;
        g_entry_wcopy[m].clear();
    }
}

int flowgnn_entry_set_devices(int n_devices, const int* device_ids) {
    if (n_devices < 1 || !device_ids) return FLOWGNN_ERR_ARG;
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    entry_drop_groups();
    g_entry_devices.assign(device_ids, device_ids + n_devices);
    return FLOWGNN_OK;
}

int flowgnn_entry_set_pipeline(int chunks_per_engine) {
    if (chunks_per_engine < 0 || chunks_per_engine > 64) return FLOWGNN_ERR_ARG;
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    if ((g_entry_pipeline == 1) != (chunks_per_engine == 1)) entry_drop_groups();  // the engine count of a one-device list changes
    g_entry_pipeline = chunks_per_engine;
    return FLOWGNN_OK;
}

int flowgnn_entry_set_option(int model, const char* key, double value) {
    if (model < 0 || model >= 6 || !key) return FLOWGNN_ERR_ARG;
    if (fg::option_index(key) < 0) return FLOWGNN_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    bool found = false;
    for (auto& kv : g_entry_options[model])
        if (kv.first == key) { kv.second = value; found = true; }
    if (!found) g_entry_options[model].emplace_back(key, value);
    if (g_entry_group[model]) {
        g_entry_wcopy[model].clear();
        return flowgnn_group_set_option(g_entry_group[model], key, value);
    }
    return FLOWGNN_OK;
}

int flowgnn_entry_set_pooling(int model, int mode) {
    if (model < 0 || model >= 6 || mode < FLOWGNN_POOL_MEAN || mode > FLOWGNN_POOL_MAX) return FLOWGNN_ERR_ARG;
    if (mode != FLOWGNN_POOL_MEAN && (model == FLOWGNN_MODEL_PNA || model == FLOWGNN_MODEL_DGN)) {
        fg::set_last_error("flowgnn_entry_set_pooling: PNA and DGN read the pooled vector through an MLP head that was trained on the mean");
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    if (g_entry_group[model]) {  // (remembered only once the engines have accepted it: a refused mode must not reach a later group)
        const int rc = flowgnn_group_set_pooling(g_entry_group[model], mode);
        if (rc) return rc;
    }
    g_entry_pooling[model] = mode;
    return FLOWGNN_OK;
}

int flowgnn_entry_set_gin_eps(int model, const float* eps) {
    if (model < 0 || model >= 6) return FLOWGNN_ERR_ARG;
    if (model != FLOWGNN_MODEL_GIN && model != FLOWGNN_MODEL_GIN_VN) {
        fg::set_last_error("flowgnn_entry_set_gin_eps: only GIN and GIN-VN have the (1 + eps) self term");
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (eps)
        for (int l = 0; l < 5; l++)
            if (!std::isfinite(eps[l])) {
                fg::set_last_error("flowgnn_entry_set_gin_eps: a value is not finite");
                return FLOWGNN_ERR_ARG;
            }
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    if (g_entry_group[model]) {  // (remembered only once the engines have accepted it)
        const int rc = flowgnn_group_set_gin_eps(g_entry_group[model], eps);
        if (rc) return rc;
    }
    g_entry_eps_on[model] = eps != nullptr;
    for (int l = 0; l < 5; l++) g_entry_eps[model][l] = eps ? eps[l] : 0.0f;
    return FLOWGNN_OK;
}

static int compute_graphs_generic(int model, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                                  const int* reload_weights, float* out, const int* node_feature, const float* node_eigen,
                                  const int* edge_list, const int* edge_attr, int ntens, const float* const* tens,
                                  const size_t* tens_elems, int num_tasks = 1) {
    if (num_graphs < 0 || num_tasks < 1) return FLOWGNN_ERR_ARG;
    if (num_graphs == 0) return FLOWGNN_OK;
    if (!nums_of_nodes || !nums_of_edges || !reload_weights || !out || !node_feature) return FLOWGNN_ERR_ARG;
    for (int i = 0; i < ntens; i++)
        if (!tens[i]) return FLOWGNN_ERR_ARG;
    if (!reload_weights[0]) return FLOWGNN_ERR_ARG;  // the reference would index weight set -1
    std::lock_guard<std::mutex> lock(g_entry_mutex);
    flowgnn_group*& grp = g_entry_group[model];
    if (!grp) {
        if (g_entry_devices.empty()) fg::read_environment(nullptr, &g_entry_devices);
        // one listed device: THREE engines on it, so that a large batch's host-side work (narrowing the arrays for the transfer, packing
        // tiles) and its host -> device copies run under the other engines' kernels (two engines: 13.4 ms per 2^18 molhiv graphs, three:
        // 11.8 -- one engine's host phase per range is longer than another's kernels for a range)
        std::vector<int> devs = g_entry_devices;
        if (devs.size() == 1 && g_entry_pipeline != 1) { devs.push_back(devs[0]); devs.push_back(devs[0]); }
        int rc = flowgnn_create_multi(model, (int)devs.size(), devs.data(), &grp);
        if (rc) return rc;
        for (auto& kv : g_entry_options[model]) {
            rc = flowgnn_group_set_option(grp, kv.first.c_str(), kv.second);
            if (rc) return rc;
        }
        if (g_entry_pooling[model] != FLOWGNN_POOL_MEAN) {
            rc = flowgnn_group_set_pooling(grp, g_entry_pooling[model]);
            if (rc) return rc;
        }
        if (g_entry_eps_on[model]) {
            rc = flowgnn_group_set_gin_eps(grp, g_entry_eps[model]);
            if (rc) return rc;
        }
        g_entry_wcopy[model].clear();
    }
    if (grp->num_tasks != num_tasks) {
        int rc = flowgnn_group_set_num_tasks(grp, num_tasks);
        if (rc) return rc;
        g_entry_wcopy[model].clear();
    }
    long long noff = 0, eoff = 0;
    int set = -1, g = 0;
    const float* cur[16];
    while (g < num_graphs) {
        set++;
        int g1 = g + 1;
        while (g1 < num_graphs && !reload_weights[g1]) g1++;
        long long n = 0, m = 0;
        for (int i = g; i < g1; i++) { n += nums_of_nodes[i]; m += nums_of_edges[i]; }
        for (int i = 0; i < ntens; i++) cur[i] = tens[i] + (size_t)set * tens_elems[i];
        int rc = FLOWGNN_OK;
        if (!same_weights(model, ntens, cur, tens_elems)) {
            g_entry_wcopy[model].clear();
            rc = flowgnn_group_set_weights(grp, ntens, cur);
            if (rc) return rc;
            remember_weights(model, ntens, cur, tens_elems);
        }
        // ranges per engine: by the size of the host arrays (~48 MB per range, at most 8 per engine); a small batch is ONE range on
        // one engine (cutting it would only add launches and half-empty tiles)
        const int n_eng = flowgnn_group_size(grp);
        int chunks = g_entry_pipeline;
        bool whole = false;
        if (chunks == 0) {
            const double bytes = (double)n * (36.0 + (node_eigen ? 16.0 : 0.0)) + (double)m * (8.0 + (edge_attr ? 12.0 : 0.0));
            const int want = (int)(bytes / 48.0e6);  // ranges in all
            whole = want < 2 && (int)g_entry_devices.size() == 1;
            chunks = (want + n_eng - 1) / n_eng;
            if (chunks < 1) chunks = 1;
            if (chunks > 8) chunks = 8;
        }
        if (whole) {  // everything on engine 0
            flowgnn_engine* e0 = flowgnn_group_engine(grp, 0);
            grp->err.clear();
            grp->batch_valid = false;  // engine 0 is about to hold this range, whatever a flowgnn_group_set_batch left
            rc = flowgnn_set_batch(e0, g1 - g, nums_of_nodes + g, nums_of_edges + g, node_feature + noff * 9,
                                   edge_list ? edge_list + eoff * 2 : nullptr, edge_attr ? edge_attr + eoff * 3 : nullptr,
                                   node_eigen ? node_eigen + noff * 4 : nullptr);
            if (!rc) rc = flowgnn_run(e0);
            if (!rc) rc = flowgnn_get_results(e0, out + (size_t)g * num_tasks);
            if (rc) { grp->err = flowgnn_last_error(e0); return rc; }
        } else {
            rc = flowgnn_group_compute(grp, g1 - g, nums_of_nodes + g, nums_of_edges + g, node_feature + noff * 9,
                                       edge_list ? edge_list + eoff * 2 : nullptr, edge_attr ? edge_attr + eoff * 3 : nullptr,
                                       node_eigen ? node_eigen + noff * 4 : nullptr, out + (size_t)g * num_tasks, chunks);
            if (rc) return rc;
        }
        noff += n;
        eoff += m;
        g = g1;
    }
    return FLOWGNN_OK;
}

int GIN_compute_graphs_mt(int num_graphs, int* nums_of_nodes, int* nums_of_edges, int* reload_weights, float* out,
                          int* node_feature_in, int* edge_list_in, int* edge_attr_in, float* node_embedding_weight_in,
                          float* edge_embedding_weight_in, float* node_mlp_1_weights, float* node_mlp_1_bias,
                          float* node_mlp_2_weights, float* node_mlp_2_bias, float* graph_pred_weights_in,
                          float* graph_pred_bias_in, int num_tasks) {
    const float* t[8] = {node_embedding_weight_in, edge_embedding_weight_in, node_mlp_1_weights, node_mlp_1_bias,
                         node_mlp_2_weights,       node_mlp_2_bias,          graph_pred_weights_in, graph_pred_bias_in};
    if (num_tasks < 1) return FLOWGNN_ERR_ARG;
    const int T = num_tasks;
    const size_t sz[8] = {173 * 100, 5 * 13 * 100, 5 * 200 * 100, 5 * 200, 5 * 100 * 200, 5 * 100, (size_t)T * 100, (size_t)T};
    return compute_graphs_generic(FLOWGNN_MODEL_GIN, num_graphs, nums_of_nodes, nums_of_edges, reload_weights, out,
                                  node_feature_in, nullptr, edge_list_in, edge_attr_in, 8, t, sz, T);
}

// The reference's symbol is `void`: a caller that ignores the status must not read an untouched buffer as results, so a refusal also
// fills `out` with NaN and says why on stderr (once per process).  The environment is asked on every call (getenv is cheap), so
// unsetting the variable in the same process clears the refusal.
static int refuse_stale_num_task(const char* symbol, float* out, int num_graphs) {
    bool stale = false;
    fg::read_environment(nullptr, nullptr, &stale);
    if (!stale) return FLOWGNN_OK;
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: FLOWGNN_NUM_TASK is set in the environment but no longer read -- call %s_mt(..., num_tasks) (include/flowgnn.h) or unset it", symbol, symbol);
    fg::set_last_error(msg);
    static std::atomic<bool> said{false};
    if (!said.exchange(true)) fprintf(stderr, "flowgnn: %s; the output buffer is filled with NaN\n", msg);
    if (out)
        for (int g = 0; g < num_graphs; g++) out[g] = std::numeric_limits<float>::quiet_NaN();
    return FLOWGNN_ERR_UNSUPPORTED;
}

int GIN_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges, int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in, int* edge_attr_in, float* node_embedding_weight_in,
                       float* edge_embedding_weight_in, float* node_mlp_1_weights, float* node_mlp_1_bias,
                       float* node_mlp_2_weights, float* node_mlp_2_bias, float* graph_pred_weights_in,
                       float* graph_pred_bias_in) {
    if (int rc = refuse_stale_num_task("GIN_compute_graphs", out, num_graphs)) return rc;
    return GIN_compute_graphs_mt(num_graphs, nums_of_nodes, nums_of_edges, reload_weights, out, node_feature_in, edge_list_in,
                                 edge_attr_in, node_embedding_weight_in, edge_embedding_weight_in, node_mlp_1_weights, node_mlp_1_bias,
                                 node_mlp_2_weights, node_mlp_2_bias, graph_pred_weights_in, graph_pred_bias_in, 1);
}

int GCN_compute_graphs_mt(int num_graphs, int* nums_of_nodes, int* nums_of_edges, int* reload_weights, float* out,
                          int* node_feature_in, int* edge_list_in, int* edge_attr_in, float* node_embedding_weight_in,
                          float* edge_embedding_weight_in, float* convs_weight_in, float* convs_bias_in,
                          float* convs_root_emb_weight_in, float* bn_weight_in, float* bn_bias_in, float* bn_mean_in,
                          float* bn_var_in, float* graph_pred_weights_in, float* graph_pred_bias_in, int num_tasks) {
    if (num_tasks < 1) return FLOWGNN_ERR_ARG;
    const float* t[11] = {node_embedding_weight_in, edge_embedding_weight_in, convs_weight_in, convs_bias_in,
                          convs_root_emb_weight_in, bn_weight_in, bn_bias_in, bn_mean_in, bn_var_in,
                          graph_pred_weights_in, graph_pred_bias_in};
    const int T = num_tasks;
    const size_t sz[11] = {173 * 100, 5 * 13 * 100, 5 * 100 * 100, 500, 500, 500, 500, 500, 500, (size_t)T * 100, (size_t)T};
    return compute_graphs_generic(FLOWGNN_MODEL_GCN, num_graphs, nums_of_nodes, nums_of_edges, reload_weights, out,
                                  node_feature_in, nullptr, edge_list_in, edge_attr_in, 11, t, sz, T);
}

int GCN_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges, int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in, int* edge_attr_in, float* node_embedding_weight_in,
                       float* edge_embedding_weight_in, float* convs_weight_in, float* convs_bias_in,
                       float* convs_root_emb_weight_in, float* bn_weight_in, float* bn_bias_in, float* bn_mean_in,
                       float* bn_var_in, float* graph_pred_weights_in, float* graph_pred_bias_in) {
    if (int rc = refuse_stale_num_task("GCN_compute_graphs", out, num_graphs)) return rc;
    return GCN_compute_graphs_mt(num_graphs, nums_of_nodes, nums_of_edges, reload_weights, out, node_feature_in, edge_list_in,
                                 edge_attr_in, node_embedding_weight_in, edge_embedding_weight_in, convs_weight_in, convs_bias_in,
                                 convs_root_emb_weight_in, bn_weight_in, bn_bias_in, bn_mean_in, bn_var_in, graph_pred_weights_in,
                                 graph_pred_bias_in, 1);
}

int PNA_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges, int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in, float* node_embedding_weight_in,
                       float* node_conv_weights_in, float* node_conv_bias_in, float* graph_mlp_1_weights_in,
                       float* graph_mlp_1_bias_in, float* graph_mlp_2_weights_in, float* graph_mlp_2_bias_in,
                       float* graph_mlp_3_weights_in, float* graph_mlp_3_bias_in, float* avg_deg_in) {
    const float* t[10] = {node_embedding_weight_in, node_conv_weights_in, node_conv_bias_in, graph_mlp_1_weights_in,
                          graph_mlp_1_bias_in, graph_mlp_2_weights_in, graph_mlp_2_bias_in, graph_mlp_3_weights_in,
                          graph_mlp_3_bias_in, avg_deg_in};
    static const size_t sz[10] = {173 * 80, 4 * 80 * 3 * 4 * 80, 4 * 80, 40 * 80, 40, 20 * 40, 20, 20, 1, 1};
    return compute_graphs_generic(FLOWGNN_MODEL_PNA, num_graphs, nums_of_nodes, nums_of_edges, reload_weights, out,
                                  node_feature_in, nullptr, edge_list_in, nullptr, 10, t, sz);
}

int DGN_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges, int* reload_weights, float* out,
                       int* node_feature_in, float* node_eigen_in, int* edge_list_in,
                       float* embedding_h_atom_embedding_list_weights_in,
                       float* layers_posttrans_fully_connected_0_linear_weight_in,
                       float* layers_posttrans_fully_connected_0_linear_bias_in, float* MLP_layer_FC_layers_0_weight_in,
                       float* MLP_layer_FC_layers_0_bias_in, float* MLP_layer_FC_layers_1_weight_in,
                       float* MLP_layer_FC_layers_1_bias_in, float* MLP_layer_FC_layers_2_weight_in,
                       float* MLP_layer_FC_layers_2_bias_in) {
    const float* t[9] = {embedding_h_atom_embedding_list_weights_in,
                         layers_posttrans_fully_connected_0_linear_weight_in,
                         layers_posttrans_fully_connected_0_linear_bias_in,
                         MLP_layer_FC_layers_0_weight_in, MLP_layer_FC_layers_0_bias_in, MLP_layer_FC_layers_1_weight_in,
                         MLP_layer_FC_layers_1_bias_in, MLP_layer_FC_layers_2_weight_in, MLP_layer_FC_layers_2_bias_in};
    static const size_t sz[9] = {9 * 119 * 100, 4 * 100 * 200, 4 * 100, 50 * 100, 50, 25 * 50, 25, 25, 1};
    if (num_graphs > 0 && !node_eigen_in) return FLOWGNN_ERR_ARG;
    return compute_graphs_generic(FLOWGNN_MODEL_DGN, num_graphs, nums_of_nodes, nums_of_edges, reload_weights, out,
                                  node_feature_in, node_eigen_in, edge_list_in, nullptr, 9, t, sz);
}

int GAT_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges, int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in, float* scoring_fn_target_in, float* scoring_fn_source_in,
                       float* linear_proj_weights_in, float* skip_proj_weights_in, float* graph_pred_weights_in,
                       float* graph_pred_bias_in) {
    const float* t[6] = {scoring_fn_target_in, scoring_fn_source_in, linear_proj_weights_in, skip_proj_weights_in,
                         graph_pred_weights_in, graph_pred_bias_in};
    static const size_t sz[6] = {5 * 4 * 16, 5 * 4 * 16, 5 * 4 * 16 * 4 * 16, 5 * 4 * 16 * 4 * 16, 16, 1};
    return compute_graphs_generic(FLOWGNN_MODEL_GAT, num_graphs, nums_of_nodes, nums_of_edges, reload_weights, out,
                                  node_feature_in, nullptr, edge_list_in, nullptr, 6, t, sz);
}

}  // extern "C"
