// host_main.cpp -- command-line host for the MI355X engine, the counterpart of the reference's per-model
// OpenCL host (GIN/src/host.cc): load the model's .bin weights, read a graph pack in the reference's on-disk
// layout, run the whole dataset as ONE batched launch NUM_TRIALS times, write HLS_output.txt.
//
//   host <MODEL> [--graphs DIR] [--weights DIR] [--num-graphs N] [--trials T] [--out FILE] [--node-logits FILE] [--attention FILE [--attention-layers MASK]] [--device D | --devices D0,D1,..] [--option key=value] [--numeric f32|q6.10|f16] [--eps] [--ogb-vn] [--attn-pool] [--set2set [--set2set-steps N]] [--jk last|sum] [--residual] [--emb-dim 100|300] [--num-layer N] [--eig DIR | --compute-eig] [XCLBIN]
//
//   MODEL        GIN | GIN-VN | GCN | GAT | PNA | DGN
//   --graphs     directory holding graph_info/ and graph_bin/      (default ../graphs, host.cc:14-15)
//   --weights    directory holding the model's .bin files          (default ., host_load.cc:24)
//   --num-graphs graph count; default = <graphs>/dataset_size.txt, else ../common/includes/dataset/dataset_size.txt
//                (the reference compiles it in: common/includes/dataset/dataset.hpp)
//   --trials     launches to time                                   (default 25 = NUM_TRIALS, host.h:8)
//   --out        result file                                        (default HLS_output.txt, host.cc:213)
//   --node-logits one more run behind the timed ones, with flowgnn_set_node_logits on: one line per node, NUM_TASK values (GIN, GIN-VN, GCN, GAT)
//   --attention  one more run behind the timed ones, with flowgnn_set_attention on (GAT): one line per selected layer and edge,
//                `layer edge h0 h1 h2 h3`, edges in the pack's order; --attention-layers: the layer mask (default 16, the last layer)
//   --eps        GIN / GIN-VN: read gin_ep1_eps_dim100.bin (five LE float32) from the weights directory and apply it (flowgnn_set_gin_eps);
//                without the flag the file stays ignored, as in the reference
//   --ogb-vn     GIN: read gin_ep1_virtualnode_dim100.bin (161 300 LE float32: vn_embedding, w1, b1, w2, b2) from the weights directory and
//                run OGB's virtual node (flowgnn_set_ogb_virtual_node) -- an exported gin-virtual checkpoint; usually together with --eps
//                (with --emb-dim 300: gin_ep1_virtualnode_dim300.bin, 1 443 900 floats, through flowgnn_set_ogb_virtual_node_dim);
//                GCN: the same from gcn_ep1_virtualnode_dim100.bin (flowgnn_set_gcn_virtual_node) -- an exported gcn-virtual checkpoint
//                (with --emb-dim 300: gcn_ep1_virtualnode_dim300.bin, through flowgnn_set_gcn_virtual_node_dim)
//   --attn-pool  GIN, GCN with --emb-dim 300: read gin_ep1_attnpool_dim300.bin / gcn_ep1_attnpool_dim300.bin (181 200 LE float32: w1, b1, w2)
//                from the weights directory and run OGB's graph_pooling="attention" readout (flowgnn_set_attention_pooling)
//   --set2set    GIN, GCN with --emb-dim 300: read gin_ep1_set2set_dim300.bin / gcn_ep1_set2set_dim300.bin (LE float32: w_ih, w_hh, b_ih, b_hh,
//                head_w, head_b; 1 082 400 + 601 per task of --num-tasks) from the weights directory and run OGB's graph_pooling="set2set"
//                readout (flowgnn_set_set2set_pooling) with --set2set-steps processing steps (default 2, OGB's); refused with --attn-pool
//   --jk, --residual   GIN or GCN with --emb-dim 300: OGB's GNN(JK="sum") and GNN(residual=True) (flowgnn_set_jk_residual; GCN: flowgnn_set_model_jk_residual).  Neither is in the weights
//                directory -- they add no parameter -- so they are given here: the flags the checkpoint was trained with
//   --emb-dim    GCN: 300 = OGB's default width (flowgnn_set_model_emb_dim), gcn_ep1_dim300.weights.all.bin is read.
//                GIN: 300 = OGB's default width (flowgnn_set_emb_dim): the weights directory's dim300 files are read (with --eps,
//                gin_ep1_eps_dim300.bin); 100 (default) = the reference's width.  With --numeric, 300 sends the mode through
//                flowgnn_group_set_numeric_mode_dim: GIN takes f16 at that width (beside --eps, --ogb-vn and --attn-pool as before);
//                GCN: through flowgnn_group_set_model_numeric_mode_dim, `host GCN --emb-dim 300 --numeric f16 [--ogb-vn] [--jk sum]
//                [--residual]` -- stages 0..3 with one f16 rounding of each operand of the layer's product
//   --num-layer  GIN or GCN with --emb-dim 300: OGB's num_layer, 2 .. 8 (flowgnn_set_num_layers; default 5).  The weights directory's files
//                keep their names and hold N layers (with --eps N floats, with --ogb-vn N - 1 updates); a file of another depth is refused
//   --numeric    f32 (default), q6.10 or f16.  `host PNA --numeric f16` sends PNA's f16 mode through
//                flowgnn_group_set_model_numeric_mode_dim at FLOWGNN_EMB_DIM_PNA (80): one f16 rounding of each operand of the layer's
//                320 -> 3 x 80 contraction, one MFMA per product
//                `host DGN --numeric f16` sends DGN's f16 mode through flowgnn_group_set_model_numeric_mode, the call that names the model:
//                one f16 rounding of each operand of the matrix-pipe products (both aggregates and the 200 -> 100 update), one MFMA each
//   --eig        DGN: directory holding the eigenvector text files g%d.txt                 (default eig, DGN/src/host_load.cc:178)
//   --compute-eig DGN: compute node_eigen from the graphs on the GPU (flowgnn_laplacian_eigen, on the first engine) and read no --eig DIR
//   XCLBIN       accepted and ignored, so `./host <xclbin>`-style command lines keep working
//
// Only the C ABI of include/flowgnn.h is used; no HIP or torch types here.
#include "../../include/flowgnn.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int model_id(const std::string& m) {
    if (m == "GIN") return FLOWGNN_MODEL_GIN;
    if (m == "GIN-VN" || m == "GIN_VN") return FLOWGNN_MODEL_GIN_VN;
    if (m == "GCN") return FLOWGNN_MODEL_GCN;
    if (m == "GAT") return FLOWGNN_MODEL_GAT;
    if (m == "PNA") return FLOWGNN_MODEL_PNA;
    if (m == "DGN") return FLOWGNN_MODEL_DGN;
    return -1;
}

template <typename T>
static bool read_exact(const std::string& path, std::vector<T>& dst, size_t start, size_t count) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const bool ok = fread(dst.data() + start, sizeof(T), count, f) == count;
    fclose(f);
    return ok;
}

// floats in a file, -1: it cannot be opened
static long file_floats(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return -1;
    long n = -1;
    if (fseek(f, 0, SEEK_END) == 0) n = ftell(f) / (long)sizeof(float);
    fclose(f);
    return n;
}

static long read_count_file(const std::string& path) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return -1;
    long n = -1;
    if (fscanf(f, "%ld", &n) != 1) n = -1;
    fclose(f);
    return n;
}

// DGN/src/host_load.cc:201-215: "tensor([[a, b,c,d],\n [..]])" -- take the numbers in order, 4 per node
static bool read_eig_txt(const std::string& path, std::vector<float>& eig, size_t start_node, int n) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return false;
    std::string txt;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) txt.append(buf, got);
    fclose(f);
    const char* p = txt.c_str();
    size_t k = 0;
    while (*p && k < (size_t)n * 4) {
        if ((*p >= '0' && *p <= '9') || ((*p == '-' || *p == '+' || *p == '.') && p[1] >= '0' && p[1] <= '9')) {
            char* end;
            eig[start_node * 4 + k++] = strtof(p, &end);
            p = end;
        } else {
            p++;
        }
    }
    return k == (size_t)n * 4;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "Usage: %s <GIN|GIN-VN|GCN|GAT|PNA|DGN> [--graphs DIR] [--weights DIR] [--num-graphs N] [--trials T] "
                        "[--out FILE] [--embeddings FILE] [--node-embeddings FILE] [--node-logits FILE] [--attention FILE [--attention-layers MASK]] [--device D | --devices D0,D1,..] [--option key=value] [--numeric f32|q6.10|f16] [--pooling mean|sum|max] [--eps] [--ogb-vn] [--attn-pool] [--set2set [--set2set-steps N]] [--jk last|sum] [--residual] [--emb-dim 100|300] [--num-layer N] [--num-tasks T] [--eig DIR | --compute-eig] [XCLBIN File]\n", argv[0]);
        return EXIT_FAILURE;
    }
    const std::string model = argv[1];
    const int mid = model_id(model);
    if (mid < 0) { fprintf(stderr, "unknown model %s\n", model.c_str()); return EXIT_FAILURE; }
    std::string graphs = "../graphs", wdir = ".", out_path = "HLS_output.txt", eig_dir = "eig", emb_path, nemb_path, nlog_path, attn_path;
    long num_graphs = -1;
    int attn_mask = 16;
    int trials = 25, numeric = FLOWGNN_NUMERIC_F32, num_tasks = 1, pooling = FLOWGNN_POOL_MEAN, emb_dim = FLOWGNN_EMB_DIM_REFERENCE;
    bool use_eps = false, use_ogb_vn = false, use_attn_pool = false, use_set2set = false, compute_eig = false;
    int set2set_steps = 2, jk = FLOWGNN_JK_LAST, residual = 0, num_layer = FLOWGNN_NUM_LAYERS_DEFAULT;
    std::vector<int> devices;
    std::vector<std::pair<std::string, double>> options;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&](const char* what) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", what); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (a == "--graphs") graphs = next("--graphs");
        else if (a == "--weights") wdir = next("--weights");
        else if (a == "--eig") eig_dir = next("--eig");
        else if (a == "--num-graphs") num_graphs = atol(next("--num-graphs"));
        else if (a == "--trials") trials = atoi(next("--trials"));
        else if (a == "--out") out_path = next("--out");
        else if (a == "--node-logits") nlog_path = next("--node-logits");  // the per-node terms of the readout, one line of NUM_TASK values per node
        else if (a == "--attention") attn_path = next("--attention");  // GAT's attention coefficients, one line per selected layer and edge
        else if (a == "--attention-layers") attn_mask = (int)strtol(next("--attention-layers"), nullptr, 0);
        else if (a == "--node-embeddings") nemb_path = next("--node-embeddings");  // the rows that pool is taken over, one line of dim values per node
        else if (a == "--embeddings") emb_path = next("--embeddings");  // the per-graph pooled embeddings, one line of dim values per graph
        else if (a == "--device") { devices.clear(); devices.push_back(atoi(next("--device"))); }
        else if (a == "--devices") {  // e.g. 0,1,2,3,4,5,6,7: the batch is cut by sum(N + E), one engine + host thread per device
            devices.clear();
            for (const char* c = next("--devices"); *c;) {
                devices.push_back(atoi(c));
                while (*c && *c != ',') c++;
                if (*c == ',') c++;
            }
        }
        else if (a == "--option") {  // key=value, flowgnn_set_option (e.g. gin_resident=0)
            const std::string kv = next("--option");
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "--option wants key=value\n"); return EXIT_FAILURE; }
            options.emplace_back(kv.substr(0, eq), atof(kv.c_str() + eq + 1));
        }
        else if (a == "--num-tasks") num_tasks = atoi(next("--num-tasks"));  // NUM_TASK of the readout (GIN/src/dcl.h:25), GIN / GIN-VN / GCN
        else if (a == "--emb-dim") emb_dim = atoi(next("--emb-dim"));  // GIN: 300 = OGB's default width (flowgnn_set_emb_dim), the dim300 files of the weights directory
        else if (a == "--num-layer") num_layer = atoi(next("--num-layer"));  // OGB's num_layer (flowgnn_set_num_layers; GIN, GCN at --emb-dim 300)
        else if (a == "--numeric") {
            const std::string m = next("--numeric");
            numeric = m == "q6.10" ? FLOWGNN_NUMERIC_Q6_10 : m == "f16" ? FLOWGNN_NUMERIC_F16 : FLOWGNN_NUMERIC_F32;
        }
        else if (a == "--pooling") {  // the readout's pooling (flowgnn_set_pooling; GIN / GIN-VN / GCN / GAT)
            const std::string m = next("--pooling");
            if (m != "mean" && m != "sum" && m != "max") { fprintf(stderr, "--pooling wants mean, sum or max\n"); return EXIT_FAILURE; }
            pooling = m == "sum" ? FLOWGNN_POOL_SUM : m == "max" ? FLOWGNN_POOL_MAX : FLOWGNN_POOL_MEAN;
        }
        else if (a == "--compute-eig") compute_eig = true;  // DGN: node_eigen from the graphs themselves (flowgnn_laplacian_eigen), no --eig DIR
        else if (a == "--eps") use_eps = true;  // the trained eps of the weights directory (flowgnn_set_gin_eps; GIN / GIN-VN)
        else if (a == "--attn-pool") use_attn_pool = true;  // OGB's attention readout from the weights directory (flowgnn_set_attention_pooling)
        else if (a == "--set2set") use_set2set = true;  // OGB's set2set readout from the weights directory (flowgnn_set_set2set_pooling)
        else if (a == "--set2set-steps") set2set_steps = atoi(next("--set2set-steps"));
        else if (a == "--jk") {  // OGB's JK (flowgnn_set_jk_residual / flowgnn_set_model_jk_residual; GIN, GCN at --emb-dim 300)
            const std::string m = next("--jk");
            if (m != "last" && m != "sum") { fprintf(stderr, "--jk wants last or sum\n"); return EXIT_FAILURE; }
            jk = m == "sum" ? FLOWGNN_JK_SUM : FLOWGNN_JK_LAST;
        }
        else if (a == "--residual") residual = 1;  // OGB's residual=True (the same calls; GIN, GCN at --emb-dim 300)
        else if (a == "--ogb-vn") use_ogb_vn = true;  // OGB's virtual node from the weights directory (GIN: flowgnn_set_ogb_virtual_node, GCN: flowgnn_set_gcn_virtual_node)
        // anything else (e.g. an .xclbin path) is ignored
    }
    if (use_set2set && use_attn_pool) { fprintf(stderr, "--set2set and --attn-pool: a model has one readout\n"); return EXIT_FAILURE; }
    if (num_graphs < 0) num_graphs = read_count_file(graphs + "/dataset_size.txt");
    if (num_graphs < 0) num_graphs = read_count_file("../common/includes/dataset/dataset_size.txt");
    if (num_graphs < 0) { fprintf(stderr, "graph count unknown: pass --num-graphs or provide dataset_size.txt\n"); return EXIT_FAILURE; }

    printf("\n******* This is the MI355X host for the %s model *******\n", model.c_str());
    if (devices.empty()) devices.push_back(0);
    flowgnn_group* eng = nullptr;  // one engine per listed device behind one handle (a single device is the common case)
    int rc = flowgnn_create_multi(mid, (int)devices.size(), devices.data(), &eng);
    if (rc) { fprintf(stderr, "flowgnn_create_multi failed: %d %s\n", rc, flowgnn_group_last_error(nullptr)); return EXIT_FAILURE; }
    for (auto& kv : options) {
        rc = flowgnn_group_set_option(eng, kv.first.c_str(), kv.second);
        if (rc) { fprintf(stderr, "--option %s: %d %s\n", kv.first.c_str(), rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (num_tasks != 1) {
        rc = flowgnn_group_set_num_tasks(eng, num_tasks);
        if (rc) { fprintf(stderr, "--num-tasks %d: %d %s\n", num_tasks, rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (emb_dim != FLOWGNN_EMB_DIM_REFERENCE) {
        // GCN's width goes through the call that names no model (flowgnn.h); GIN keeps the call it had
        rc = mid == FLOWGNN_MODEL_GCN ? flowgnn_group_set_model_emb_dim(eng, emb_dim) : flowgnn_group_set_emb_dim(eng, emb_dim);
        if (rc) { fprintf(stderr, "--emb-dim %d: %d %s\n", emb_dim, rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (num_layer != FLOWGNN_NUM_LAYERS_DEFAULT) {  // behind the width (the depth is a choice at 300), in front of the weights (they are a depth's)
        rc = flowgnn_group_set_num_layers(eng, emb_dim, num_layer);
        if (rc) { fprintf(stderr, "--num-layer %d: %d %s\n", num_layer, rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    rc = flowgnn_group_load_weights_dir(eng, wdir.c_str());
    if (rc) { fprintf(stderr, "loading weights failed: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    if (numeric != FLOWGNN_NUMERIC_F32) {  // the reference's ap_fixed<16,6> bit patterns, or f16 MLP operands (GIN / GIN-VN)
        // --emb-dim 300: through the call that carries the width (GIN's f16 mode at that width, gin_wide_f16.hip); GCN's goes through
        // the call that names no model (gcn_wide_f16.hip), as its width did
        // PNA's f16 mode: the group's model form at the model's true width (pna_f16.hip)
        // DGN's f16 mode: the group's call that names the model (dgn_f16.hip)
        if (mid == FLOWGNN_MODEL_DGN && numeric == FLOWGNN_NUMERIC_F16) rc = flowgnn_group_set_model_numeric_mode(eng, FLOWGNN_MODEL_DGN, numeric);
        else if (mid == FLOWGNN_MODEL_PNA && numeric == FLOWGNN_NUMERIC_F16) rc = flowgnn_group_set_model_numeric_mode_dim(eng, FLOWGNN_EMB_DIM_PNA, numeric);
        else if (mid == FLOWGNN_MODEL_GCN && emb_dim != FLOWGNN_EMB_DIM_REFERENCE) rc = flowgnn_group_set_model_numeric_mode_dim(eng, emb_dim, numeric);
        else rc = emb_dim != FLOWGNN_EMB_DIM_REFERENCE ? flowgnn_group_set_numeric_mode_dim(eng, emb_dim, numeric) : flowgnn_group_set_numeric_mode(eng, numeric);
        if (rc) { fprintf(stderr, "numeric mode: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (pooling != FLOWGNN_POOL_MEAN) {
        rc = flowgnn_group_set_pooling(eng, pooling);
        if (rc) { fprintf(stderr, "--pooling: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (use_eps) {
        std::vector<float> eps((size_t)num_layer);
        const std::string path = wdir + "/gin_ep1_eps_dim" + std::to_string(emb_dim) + ".bin";
        const long have = file_floats(path);
        if (num_layer != FLOWGNN_NUM_LAYERS_DEFAULT && have >= 0 && have != num_layer) {
            fprintf(stderr, "--eps: %s holds the eps of %ld layers, and --num-layer is %d\n", path.c_str(), have, num_layer);
            return EXIT_FAILURE;
        }
        if (!read_exact(path, eps, 0, eps.size())) { fprintf(stderr, "--eps: cannot read %s floats from %s\n", num_layer == 5 ? "five" : std::to_string(num_layer).c_str(), path.c_str()); return EXIT_FAILURE; }
        rc = flowgnn_group_set_gin_eps(eng, eps.data());
        if (rc) { fprintf(stderr, "--eps: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (use_ogb_vn) {
        const bool gcn = mid == FLOWGNN_MODEL_GCN;
        const bool wide = emb_dim != FLOWGNN_EMB_DIM_REFERENCE;  // --emb-dim 300: the file of that width, through the call that carries it
        const size_t L = (size_t)num_layer - 1 /* FLOWGNN_OGB_VN_LAYERS at the default depth */, D = wide ? (size_t)emb_dim : 100, H = 2 * D;
        const size_t at[6] = {0, D, D + L * H * D, D + L * H * D + L * H, D + 2 * L * H * D + L * H, D + 2 * L * H * D + L * H + L * D};
        std::vector<float> vn(at[5]);
        const std::string path = wdir + (gcn ? "/gcn_ep1_virtualnode_dim" : "/gin_ep1_virtualnode_dim") + std::to_string(D) + ".bin";
        const char* const call = wide ? (gcn ? "flowgnn_set_gcn_virtual_node_dim" : "flowgnn_set_ogb_virtual_node_dim")
                                      : (gcn ? "flowgnn_set_gcn_virtual_node" : "flowgnn_set_ogb_virtual_node");
        const long have = file_floats(path);
        if (num_layer != FLOWGNN_NUM_LAYERS_DEFAULT && have >= 0 && (size_t)have != vn.size()) {
            fprintf(stderr, "--ogb-vn: %s holds %ld floats, and the tensors of %d updates (--num-layer %d) are %zu\n", path.c_str(), have, num_layer - 1,
                    num_layer, vn.size());
            return EXIT_FAILURE;
        }
        if (!read_exact(path, vn, 0, vn.size())) {
            fprintf(stderr, "--ogb-vn: cannot read %zu floats from %s (the tensors of %s)\n", vn.size(), path.c_str(), call);
            return EXIT_FAILURE;
        }
        if (wide)
            rc = (gcn ? flowgnn_group_set_gcn_virtual_node_dim : flowgnn_group_set_ogb_virtual_node_dim)(eng, emb_dim, vn.data() + at[0], vn.data() + at[1],
                                                                                                         vn.data() + at[2], vn.data() + at[3], vn.data() + at[4]);
        else
            rc = (gcn ? flowgnn_group_set_gcn_virtual_node : flowgnn_group_set_ogb_virtual_node)(eng, vn.data() + at[0], vn.data() + at[1], vn.data() + at[2],
                                                                                                 vn.data() + at[3], vn.data() + at[4]);
        if (rc) { fprintf(stderr, "--ogb-vn: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (use_attn_pool) {
        const size_t D = (size_t)emb_dim, H = 2 * D;
        std::vector<float> gate(H * D + 2 * H);
        const std::string path = wdir + (mid == FLOWGNN_MODEL_GCN ? "/gcn_ep1_attnpool_dim" : "/gin_ep1_attnpool_dim") + std::to_string(D) + ".bin";
        if (!read_exact(path, gate, 0, gate.size())) {
            fprintf(stderr, "--attn-pool: cannot read %zu floats from %s (the tensors of flowgnn_set_attention_pooling)\n", gate.size(), path.c_str());
            return EXIT_FAILURE;
        }
        rc = flowgnn_group_set_attention_pooling(eng, emb_dim, gate.data(), gate.data() + H * D, gate.data() + H * D + H);
        if (rc) { fprintf(stderr, "--attn-pool: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (use_set2set) {
        const size_t D = (size_t)emb_dim, T = (size_t)(num_tasks > 0 ? num_tasks : 1);
        const size_t at[7] = {0, 8 * D * D, 12 * D * D, 12 * D * D + 4 * D, 12 * D * D + 8 * D, 12 * D * D + 8 * D + T * 2 * D, 12 * D * D + 8 * D + T * (2 * D + 1)};
        std::vector<float> t(at[6]);
        const std::string path = wdir + (mid == FLOWGNN_MODEL_GCN ? "/gcn_ep1_set2set_dim" : "/gin_ep1_set2set_dim") + std::to_string(D) + ".bin";
        if (!read_exact(path, t, 0, t.size())) {
            fprintf(stderr, "--set2set: cannot read %zu floats from %s (the tensors of flowgnn_set_set2set_pooling at --num-tasks %zu)\n", t.size(), path.c_str(), T);
            return EXIT_FAILURE;
        }
        rc = flowgnn_group_set_set2set_pooling(eng, emb_dim, set2set_steps, (int)T, t.data() + at[0], t.data() + at[1], t.data() + at[2], t.data() + at[3],
                                               t.data() + at[4], t.data() + at[5]);
        if (rc) { fprintf(stderr, "--set2set: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    if (jk != FLOWGNN_JK_LAST || residual) {
        // (GCN: the model form of the call, as with --emb-dim; on a GIN engine the two are one)
        rc = model == "GCN" ? flowgnn_group_set_model_jk_residual(eng, emb_dim, jk, residual) : flowgnn_group_set_jk_residual(eng, emb_dim, jk, residual);
        if (rc) { fprintf(stderr, "--jk / --residual: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    }
    printf("\n******* Weights loading done *******\n");

    const bool vn = mid == FLOWGNN_MODEL_GIN_VN, dgn = mid == FLOWGNN_MODEL_DGN;
    std::vector<int> nn(num_graphs), ne(num_graphs), nf, el, ea;
    std::vector<float> eig;
    size_t N = 0, E = 0;
    for (long g = 1; g <= num_graphs; g++) {
        char info[512];
        snprintf(info, sizeof(info), "%s/graph_info/g%ld_info.txt", graphs.c_str(), g);
        FILE* f = fopen(info, "r");
        int n = 0, e = 0;
        if (!f || fscanf(f, "%d\n%d", &n, &e) != 2) { fprintf(stderr, "cannot read %s\n", info); return EXIT_FAILURE; }
        fclose(f);
        char base[512];
        snprintf(base, sizeof(base), "%s/graph_bin/g%ld", graphs.c_str(), g);
        const int n2 = vn ? n + 1 : n, e2 = vn ? e + 2 * n : e;  // GIN-VN/src/host.cc:133-134
        nf.resize((N + n2) * 9, 0);
        el.resize((E + e2) * 2, 0);
        ea.resize((E + e2) * 3, 0);
        if (!read_exact(std::string(base) + "_node_feature.bin", nf, N * 9, (size_t)n * 9) ||
            !read_exact(std::string(base) + "_edge_list.bin", el, E * 2, (size_t)e * 2)) {
            fprintf(stderr, "cannot read graph %ld under %s\n", g, base);
            return EXIT_FAILURE;
        }
        read_exact(std::string(base) + "_edge_attr.bin", ea, E * 3, (size_t)e * 3);  // absent for some packs: zeros
        if (vn) {  // GIN-VN/src/host_load.cc:125-153: virtual node N, edges (nd, N) and (N, nd), attributes 0
            for (int nd = 0; nd < n; nd++) {
                el[(E + e + 2 * nd) * 2 + 0] = nd; el[(E + e + 2 * nd) * 2 + 1] = n;
                el[(E + e + 2 * nd + 1) * 2 + 0] = n; el[(E + e + 2 * nd + 1) * 2 + 1] = nd;
            }
        }
        if (dgn) {
            eig.resize((N + n2) * 4, 0.0f);
            if (!compute_eig) {
                char ep[512];
                snprintf(ep, sizeof(ep), "%s/g%ld.txt", eig_dir.c_str(), g);
                if (!read_eig_txt(ep, eig, N, n)) { fprintf(stderr, "cannot read %s\n", ep); return EXIT_FAILURE; }
            }
        }
        nn[g - 1] = n2;
        ne[g - 1] = e2;
        N += n2;
        E += e2;
        if (g % 1000 == 0 || g == num_graphs) { printf("(%ld/%ld) Loading graphs ...\r", g, num_graphs); fflush(stdout); }
    }
    printf("\n******* Graphs loading done *******\n");
    if (dgn && compute_eig) {
        flowgnn_engine* first = flowgnn_group_engine(eng, 0);
        rc = flowgnn_laplacian_eigen(first, (int)num_graphs, nn.data(), ne.data(), el.data(), eig.data());
        if (rc) { fprintf(stderr, "--compute-eig: %d %s\n", rc, flowgnn_last_error(first)); return EXIT_FAILURE; }
    }

    rc = flowgnn_group_set_batch(eng, (int)num_graphs, nn.data(), ne.data(), nf.data(), el.data(), ea.data(), dgn ? eig.data() : nullptr);
    if (rc) { fprintf(stderr, "flowgnn_set_batch failed: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    rc = flowgnn_group_run(eng);  // warm-up (first-touch, code load)
    if (!rc) rc = flowgnn_group_sync(eng);
    if (rc) { fprintf(stderr, "run failed: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < trials; i++) {
        printf("(%d/%d) Computing %s ...\r", i + 1, trials, model.c_str());
        fflush(stdout);
        rc = flowgnn_group_run(eng);
        if (rc) break;
    }
    if (!rc) rc = flowgnn_group_sync(eng);
    const auto t1 = std::chrono::steady_clock::now();
    if (rc) { fprintf(stderr, "run failed: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count() / (trials > 0 ? trials : 1);
    printf("\n******* Computation done *******\n");
    // the figure run_experiments.sh derives: kernel ms for the whole dataset / graphs (run_experiments.sh:44-46)
    printf("%s: %.6f ms per launch, %.6f ms per graph, %.1f graphs/s (%ld graphs, %zu nodes, %zu edges)\n", model.c_str(), ms,
           ms / num_graphs, num_graphs / (ms * 1e-3), num_graphs, N, E);

    std::vector<float> result((size_t)num_graphs * num_tasks);
    rc = flowgnn_group_get_results(eng, result.data());
    if (rc) { fprintf(stderr, "flowgnn_get_results failed: %d\n", rc); return EXIT_FAILURE; }
    FILE* o = fopen(out_path.c_str(), "w+");
    if (!o) { fprintf(stderr, "cannot write %s\n", out_path.c_str()); return EXIT_FAILURE; }
    for (long g = 1; g <= num_graphs; g++)  // one line per task, as host.cc:213-222
        for (int t = 0; t < num_tasks; t++) fprintf(o, "g%ld: %.8f\n", g, result[(size_t)(g - 1) * num_tasks + t]);
    fclose(o);
    if (!emb_path.empty()) {
        // one more run with embeddings on, behind the timed ones: the figures and the logits above are those of a run without the flag
        const int dim = flowgnn_emb_dim(flowgnn_group_engine(eng, 0));
        std::vector<float> emb((size_t)num_graphs * dim);
        rc = flowgnn_group_set_embeddings(eng, 1);
        if (!rc) rc = flowgnn_group_run(eng);
        if (!rc) rc = flowgnn_group_get_embeddings(eng, emb.data());
        if (rc) { fprintf(stderr, "--embeddings: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
        FILE* ef = fopen(emb_path.c_str(), "w");
        if (!ef) { fprintf(stderr, "cannot write %s\n", emb_path.c_str()); return EXIT_FAILURE; }
        for (long g = 0; g < num_graphs; g++)
            for (int d = 0; d < dim; d++) fprintf(ef, d + 1 < dim ? "%.8f " : "%.8f\n", emb[(size_t)g * dim + d]);
        fclose(ef);
    }
    if (!nemb_path.empty()) {
        // likewise one more run, with node embeddings on (and graph embeddings off again)
        const int dim = flowgnn_emb_dim(flowgnn_group_engine(eng, 0));
        const size_t n_tot = N;
        std::vector<float> rows(n_tot * dim);
        rc = flowgnn_group_set_embeddings(eng, 0);
        if (!rc) rc = flowgnn_group_set_node_embeddings(eng, 1);
        if (!rc) rc = flowgnn_group_run(eng);
        if (!rc) rc = flowgnn_group_get_node_embeddings(eng, rows.data());
        if (rc) { fprintf(stderr, "--node-embeddings: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
        FILE* nf = fopen(nemb_path.c_str(), "w");
        if (!nf) { fprintf(stderr, "cannot write %s\n", nemb_path.c_str()); return EXIT_FAILURE; }
        for (size_t v = 0; v < n_tot; v++)
            for (int d = 0; d < dim; d++) fprintf(nf, d + 1 < dim ? "%.8f " : "%.8f\n", rows[v * dim + d]);
        fclose(nf);
    }
    if (!nlog_path.empty()) {
        // likewise one more run, with node logits on (and both kinds of embeddings off again)
        const size_t n_tot = N;
        std::vector<float> terms(n_tot * num_tasks);
        rc = flowgnn_group_set_embeddings(eng, 0);
        if (!rc) rc = flowgnn_group_set_node_embeddings(eng, 0);
        if (!rc) rc = flowgnn_group_set_node_logits(eng, 1);
        if (!rc) rc = flowgnn_group_run(eng);
        if (!rc) rc = flowgnn_group_get_node_logits(eng, terms.data());
        if (rc) { fprintf(stderr, "--node-logits: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
        FILE* lf = fopen(nlog_path.c_str(), "w");
        if (!lf) { fprintf(stderr, "cannot write %s\n", nlog_path.c_str()); return EXIT_FAILURE; }
        for (size_t v = 0; v < n_tot; v++)
            for (int t = 0; t < num_tasks; t++) fprintf(lf, t + 1 < num_tasks ? "%.8f " : "%.8f\n", terms[v * num_tasks + t]);
        fclose(lf);
    }
    if (!attn_path.empty()) {
        // likewise one more run, with attention on (and everything else off again)
        const size_t e_tot = E;
        size_t n_sel = 0;
        for (int l = 0; l < 5; l++) n_sel += (attn_mask >> l) & 1;
        std::vector<float> attn(n_sel * e_tot * 4);
        rc = flowgnn_group_set_embeddings(eng, 0);
        if (!rc) rc = flowgnn_group_set_node_embeddings(eng, 0);
        if (!rc && (mid == FLOWGNN_MODEL_GIN || mid == FLOWGNN_MODEL_GIN_VN || mid == FLOWGNN_MODEL_GCN || mid == FLOWGNN_MODEL_GAT))
            rc = flowgnn_group_set_node_logits(eng, 0);
        if (!rc) rc = flowgnn_group_set_attention(eng, attn_mask);
        if (!rc && n_sel == 0) { fprintf(stderr, "--attention-layers 0 selects no layer\n"); return EXIT_FAILURE; }
        if (!rc) rc = flowgnn_group_run(eng);
        if (!rc) rc = flowgnn_group_get_attention(eng, attn.data(), nullptr);
        if (rc) { fprintf(stderr, "--attention: %d %s\n", rc, flowgnn_group_last_error(eng)); return EXIT_FAILURE; }
        FILE* af = fopen(attn_path.c_str(), "w");
        if (!af) { fprintf(stderr, "cannot write %s\n", attn_path.c_str()); return EXIT_FAILURE; }
        size_t k = 0;
        for (int l = 0; l < 5; l++) {
            if (!((attn_mask >> l) & 1)) continue;
            for (size_t i = 0; i < e_tot; i++) {
                const float* a = &attn[(k * e_tot + i) * 4];
                fprintf(af, "%d %zu %.8f %.8f %.8f %.8f\n", l, i, a[0], a[1], a[2], a[3]);
            }
            k++;
        }
        fclose(af);
    }
    flowgnn_group_destroy(eng);
    return 0;
}
