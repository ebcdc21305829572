// engine.hip -- host-side engine and the C ABI declared in include/flowgnn.h.
//
// One engine = one GPU + one HIP stream + one model's weights + one resident batch.
// The reference host (GIN/src/host.cc) programs an FPGA, migrates flat buffers once and
// enqueues the kernel NUM_TRIALS times; the counterpart here is
//   flowgnn_create -> flowgnn_set_weights_* / flowgnn_load_weights_dir -> flowgnn_set_batch
//   -> N x flowgnn_run -> flowgnn_get_results.
// Several engines behind one handle: group.hip; the reference's <M>_compute_graphs symbols: entry.hip.
// The calls that configure an engine (width, numeric mode, pooling, eps, virtual nodes, readouts, JK / residual): engine_config.hip.
#include "engine_internal.h"
#include "tile_pack.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cctype>
#include <cmath>
#include <thread>

namespace fg {

// ------------------------------------------------------------------ error text
static thread_local char g_err[512] = "";
void set_hip_error(const char* what, hipError_t e, const char* file, int line) {
    snprintf(g_err, sizeof(g_err), "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
}
const char* last_error_text() { return g_err; }
void set_last_error(const char* what) { snprintf(g_err, sizeof(g_err), "%s", what); }

int read_floats(const char* dir, const char* file, size_t offset_floats, size_t count, float* dst) {
    std::string path = std::string(dir) + "/" + file;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        snprintf(g_err, sizeof(g_err), "cannot open %s", path.c_str());
        return FLOWGNN_ERR_IO;
    }
    int rc = 0;
    if (fseek(f, (long)(offset_floats * sizeof(float)), SEEK_SET) != 0 || fread(dst, sizeof(float), count, f) != count) {
        snprintf(g_err, sizeof(g_err), "short read of %zu floats at offset %zu from %s", count, offset_floats, path.c_str());
        rc = FLOWGNN_ERR_IO;
    }
    fclose(f);
    return rc;
}

int check_layer_file(const char* dir, const char* file, size_t fixed_floats, size_t per_layer_floats, int layers) {
    const std::string path = std::string(dir) + "/" + file;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return 0;  // (read_floats says so)
    long bytes = -1;
    if (fseek(f, 0, SEEK_END) == 0) bytes = ftell(f);
    fclose(f);
    if (bytes < 0 || bytes % (long)sizeof(float) != 0) return 0;
    const size_t have = (size_t)bytes / sizeof(float);
    if (have == fixed_floats + (size_t)layers * per_layer_floats) return 0;
    for (int k = 2; k <= MAX_NUM_LAYERS; k++)
        if (have == fixed_floats + (size_t)k * per_layer_floats) {
            snprintf(g_err, sizeof(g_err), "%s holds the tensors of a model %d layers deep, and the engine's depth is %d (flowgnn_set_num_layers)", path.c_str(), k, layers);
            return FLOWGNN_ERR_IO;
        }
    return 0;
}

int read_layer_floats(const char* dir, const char* file, int layers, size_t per_layer_floats, float* dst) {
    if (int rc = check_layer_file(dir, file, 0, per_layer_floats, layers)) return rc;
    return read_floats(dir, file, 0, (size_t)layers * per_layer_floats, dst);
}

// ------------------------------------------------------------------ profiler
Profiler::~Profiler() {
    for (auto& p : pending_) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : free_) (void)hipEventDestroy(e);
}
int Profiler::slot(const char* name) {
    for (size_t i = 0; i < names.size(); i++)
        if (names[i] == name) return (int)i;
    names.push_back(name);
    total_ms.push_back(0.0);
    launches.push_back(0);
    return (int)names.size() - 1;
}
hipEvent_t Profiler::get_event() {
    if (!free_.empty()) { hipEvent_t e = free_.back(); free_.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);  // a failure shows up as an invalid-handle error at the first record, reported by flowgnn_run
    return e;
}
void Profiler::begin(int slot, hipStream_t s) {
    Pending p{slot, get_event(), get_event()};
    (void)hipEventRecord(p.a, s);
    pending_.push_back(p);
}
void Profiler::end(int slot, hipStream_t s) {
    for (size_t i = pending_.size(); i-- > 0;)
        if (pending_[i].slot == slot) { (void)hipEventRecord(pending_[i].b, s); break; }
}
void Profiler::collect() {
    for (auto& p : pending_) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            total_ms[p.slot] += ms;
            launches[p.slot] += 1;
        }
        free_.push_back(p.a);
        free_.push_back(p.b);
    }
    pending_.clear();
}
void Profiler::reset() {
    collect();
    for (auto& x : total_ms) x = 0.0;
    for (auto& x : launches) x = 0;
}

// ------------------------------------------------------------------ options
// Every run-time switch of the library, with its default.  Keys ending in _ablate exist only in -DFLOWGNN_DEV builds.
struct OptionDef { const char* key; double dflt; };
static const OptionDef kOptionTable[] = {
    {"hipgraph", 0},              // 1: replay the launch sequence of resident batches of up to 2^20 nodes; 2: of any size
    {"csr_flat", 0},              // 1: global-memory index build for every graph (A/B)
    {"tile_nominal", -1},         // rows per tile of the tiled aggregation kernels (< 0: the model's default)
    {"tile_slack", -1},
    {"h2d_pack", 16},             // flowgnn_set_batch: host threads that narrow a large batch's int32 arrays for the transfer (h2d_pack.cpp); 0: plain copies
    {"tile_balance", 1},          // graph tiles of a batch of <= 8 rounds over the CUs: fewer rows per tile, whole rounds of tiles (flowgnn_set_batch)
    {"gin_resident", 1}, {"gin_binpack", 1}, {"gin_tile_build", -1}, {"gin_resident_min_fill", 0.5}, {"gin_resident_nosort", 0}, {"gin_resident_prof", 0},
    {"gin_unfused", 0}, {"gin_mfma", 16}, {"gin_split_nt", 4}, {"gin_fold_readout", 1}, {"gin_head_fold", 1},
    {"gin_agg_untiled", 0}, {"gin_agg_tile", 128},
    {"gcn_resident", 1}, {"gcn_binpack", 1}, {"gcn_tile_build", 1}, {"gcn_unfused", 0}, {"gcn_mfma", 16},
    {"gat_resident", 1}, {"gat_mfma", 16}, {"gat_fold_readout", 1}, {"gat_reference_quirk", 0},
    {"pna_resident", 1}, {"pna_binpack", 1}, {"pna_tile_build", 1}, {"pna_fused", 1}, {"pna_mfma", 16},
    {"pna_mfma_agg", 0},          // deprecated (removed in round 5, the kernel it selected is gone): accepted and ignored, so that callers' scripts keep working
    {"dgn_fused", 1}, {"dgn_mfma", 16}, {"dgn_mfma_agg", -1}, {"dgn_fold_readout", 1}, {"dgn_rowinfo_direct", 1}, {"dgn_resident", 1}, {"dgn_binpack", 1},
#ifdef FLOWGNN_DEV
    {"gcn_ablate", 0}, {"gat_ablate", 0}, {"pna_ablate", 0}, {"dgn_ablate", 0}, {"gin_pingpong", 0},
#endif
};
constexpr int kNumOptions = (int)(sizeof(kOptionTable) / sizeof(kOptionTable[0]));

int option_index(const char* key) {
    if (!key) return -1;
    for (int i = 0; i < kNumOptions; i++)
        if (strcmp(kOptionTable[i].key, key) == 0) return i;
    return -1;
}

// THE place where the library reads its environment: FLOWGNN_<KEY> seeds option <key> of every engine created afterwards
// ("f32" reads as 32, for the *_mfma switches); FLOWGNN_DEVICES / FLOWGNN_DEVICE seed the device list of the
// <M>_compute_graphs entry points (entry.hip).
static double env_number(const char* text) {
    if (strcmp(text, "f32") == 0) return 32.0;
    if (strcmp(text, "f16") == 0) return 16.0;
    return atof(text);
}
// stale_num_task: FLOWGNN_NUM_TASK (round 2's way to give the entry points NUM_TASK) is set to something other than 1.  It is no
// longer read -- NUM_TASK is an argument of the *_compute_graphs_mt symbols -- and a caller that still relies on it would get
// one task's worth of results for [T][100] weights, silently: the plain GIN / GCN entry points refuse to run instead.
void read_environment(std::vector<double>* option_values, std::vector<int>* devices, bool* stale_num_task) {
    if (stale_num_task) {
        const char* v = getenv("FLOWGNN_NUM_TASK");
        *stale_num_task = v && *v && atoi(v) != 1;
    }
    if (option_values) {
        option_values->resize(kNumOptions);
        for (int i = 0; i < kNumOptions; i++) {
            (*option_values)[i] = kOptionTable[i].dflt;
            std::string name = "FLOWGNN_";
            for (const char* c = kOptionTable[i].key; *c; c++) name += (char)toupper((unsigned char)*c);
            const char* v = getenv(name.c_str());
            if (v && *v) (*option_values)[i] = env_number(v);
        }
    }
    if (devices) {
        devices->clear();
        const char* v = getenv("FLOWGNN_DEVICES");
        if (!v || !*v) v = getenv("FLOWGNN_DEVICE");
        if (v && *v) {
            for (const char* c = v; *c;) {
                devices->push_back(atoi(c));
                while (*c && *c != ',') c++;
                if (*c == ',') c++;
            }
        }
        if (devices->empty()) devices->push_back(0);
    }
}

Options::Options() { read_environment(&v_, nullptr); }
bool Options::set(const char* key, double v) {
    const int i = option_index(key);
    if (i < 0) return false;
    v_[i] = v;
    return true;
}
bool Options::get(const char* key, double* v) const {
    const int i = option_index(key);
    if (i < 0) return false;
    if (v) *v = v_[i];
    return true;
}
double Options::num(const char* key) const {
    const int i = option_index(key);
    return i < 0 ? 0.0 : v_[i];
}

}  // namespace fg

using namespace fg;

namespace fg {
// h2d_pack.cpp
size_t h2d_pack_bytes(size_t n_nodes, size_t n_edges, bool attr, size_t* off_edges, size_t* off_attr);
void h2d_pack(const int* node_feature, const int* edge_list, const int* edge_attr, size_t n_nodes, size_t n_edges, uint8_t* dst, int threads);
void host_parallel_for(int parts, const std::function<void(int)>& fn);
// ingest.hip
void launch_ingest_pyg(const long long* x, const long long* ei, const long long* ea, int* nf, int* el, int* ea_out, const int* noff,
                       const int* eoff, int G, long long N, long long E, int* err, int x_err, int device, hipStream_t s);
// eigen.hip
void launch_laplacian_eigen(int cls, const int* list, int count, const int* noff, const int* eoff, const void* edges, long long E,
                            bool pyg, float* out, hipStream_t s);

// the packed arrays back into the reference's int32 layout (what every kernel reads): 255 / 65 535 = "did not fit" -> -1, which the
// validation on the device refuses as it would have refused the original value
__global__ __launch_bounds__(256) void unpack_batch_kernel(const uint8_t* __restrict__ nf8, const uint16_t* __restrict__ el16, const uint8_t* __restrict__ ea8,
                                                           int* __restrict__ nf, int* __restrict__ el, int* __restrict__ ea, long long n9, long long e2,
                                                           long long ne) {
    const long long stride = (long long)gridDim.x * 256 * 4;
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n9; i += stride) {  // four values per thread: n9 and e2 are padded to 16 B
        const uint32_t w = *reinterpret_cast<const uint32_t*>(nf8 + i);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k < n9) { const int v = (int)((w >> (8 * k)) & 0xFFu); nf[i + k] = v == 255 ? -1 : v; }
    }
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < e2; i += stride) {
        const uint2 w = *reinterpret_cast<const uint2*>(el16 + i);
        const int v[4] = {(int)(w.x & 0xFFFFu), (int)(w.x >> 16), (int)(w.y & 0xFFFFu), (int)(w.y >> 16)};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k < e2) el[i + k] = v[k] == 65535 ? -1 : v[k];
    }
    if (ea8)
        for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < ne; i += stride) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(ea8 + i);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i + k < ne) {
                    const int c = (int)((w >> (8 * k)) & 0xFFu);
                    int* o = ea + 3 * (i + k);
                    if (c == 255) { o[0] = -1; o[1] = 0; o[2] = 0; }
                    else { o[0] = c / 12; o[1] = (c >> 1) % 6; o[2] = c & 1; }
                }
        }
}
static void launch_unpack_batch(const uint8_t* nf8, const uint8_t* el16, const uint8_t* ea8, int* nf, int* el, int* ea, long long n, long long e, hipStream_t s) {
    const long long work = n * 9 > e * 2 ? n * 9 : e * 2;
    long long blocks = (work / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    unpack_batch_kernel<<<(int)blocks, 256, 0, s>>>(nf8, reinterpret_cast<const uint16_t*>(el16), ea8, nf, el, ea, n * 9, e * 2, e);
}

// host threads a call may use: the option's count, capped by what this process may run on (affinity mask, cgroup CPU quota)
static int host_threads(int want) {
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
        char q[32];
        long long period = 0;
        if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long long cpus = (atoll(q) + period - 1) / period;
            if (cpus >= 1 && cpus < n) n = (int)cpus;
        }
        fclose(f);
    }
    return want < n ? (want < 1 ? 1 : want) : n;
}
}  // namespace fg

// ------------------------------------------------------------------ engine object (struct flowgnn_engine: engine_internal.h)
int use_device(flowgnn_engine* e) {
    FG_HIP_TRY(hipSetDevice(e->device));
    return 0;
}

// what every call that changes what the launched kernels read starts with: the engine's device, no recorded launch sequence, an idle stream
int begin_change(flowgnn_engine* e) {
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();
    if (e->stream) EHIP_TRY(e, hipStreamSynchronize(e->stream));
    return 0;
}

// index build (when the model's next forward needs the CSR) + forward pass, on the engine's stream; the state the model decides
// on (exact / keep_h / numeric mode) must be set before
static int engine_forward(flowgnn_engine* e) {
    if (e->model->needs_csr(e->db)) {
        ProfScope p(e->prof, "build_csr", e->stream);
        const bool flat = e->opts.on("csr_flat");  // A/B: force the global path
        launch_build_csr(e->db.b, e->db.csr, e->has_attr, flat ? (1 << 30) : e->max_nodes, flat ? (1 << 30) : e->max_edges, e->stream);
        e->db.csr_built = true;
    }
    return e->model->forward(e->db, e->prof, e->stream);
}
// taps that read the CSR (flowgnn_get_csr, the stand-alone aggregation kernels): build it if no run of this batch has
static void ensure_csr(flowgnn_engine* e) {
    if (e->db.csr_built || e->G == 0) return;
    launch_build_csr(e->db.b, e->db.csr, e->has_attr, e->max_nodes, e->max_edges, e->stream);
    e->db.csr_built = true;
}

// (The optional per-run outputs, fg::OutSlot, and the ONE list of them, kOutputs: engine_internal.h.)

// One output after anything it follows has changed (switch, caller's buffer, batch): with the output on and no caller's buffer, the
// engine's own buffer holds what the resident batch needs; the DeviceBatch pointer is the target, or null without a batch
static int place(flowgnn_engine* e, const Output& o) {
    fg::OutSlot& s = e->*o.slot;
    const bool on = e->batch_ready && is_on(e, o);
    if (on && !s.user) {
        const size_t need = sizeof(float) * o.floats(e);
        if (!s.own.holds(need)) {
            if (e->stream) EHIP_TRY(e, hipStreamSynchronize(e->stream));  // (a run in flight may still write the old one)
            if (s.last == s.own.p) s.last = nullptr;
            EHIP_TRY(e, s.own.reserve(need, false));  // no headroom: one batch's size, kept across batches
        }
    }
    e->db.*o.field = s.target(on);
    return FLOWGNN_OK;
}
// ... and the attention coefficients: two outputs, and the mask the models read
static int place_attention(flowgnn_engine* e) {
    if (int rc = place(e, kOutputs[OUT_ATTN_E])) return rc;
    if (int rc = place(e, kOutputs[OUT_ATTN_S])) return rc;
    e->db.attn_mask = e->batch_ready ? e->attn_mask : 0;
    return FLOWGNN_OK;
}

// The DeviceBatch's output pointers and attention mask as they are, put back when the scope ends: a pass that is to fill other
// buffers than the next run's (the exact re-run), or none (a tap's pass), installs its own in between
struct KeepOutputFields {
    DeviceBatch& db;
    float* ptr[sizeof(kOutputs) / sizeof(kOutputs[0])];
    const int mask;
    explicit KeepOutputFields(DeviceBatch& d) : db(d), mask(d.attn_mask) {
        for (size_t i = 0; i < sizeof(ptr) / sizeof(ptr[0]); i++) ptr[i] = db.*kOutputs[i].field;
    }
    ~KeepOutputFields() {
        for (size_t i = 0; i < sizeof(ptr) / sizeof(ptr[0]); i++) db.*kOutputs[i].field = ptr[i];
        db.attn_mask = mask;
    }
};

extern "C" {

int flowgnn_embedding_dim(int model) {
    switch (model) {
        case FLOWGNN_MODEL_GIN: case FLOWGNN_MODEL_GIN_VN: case FLOWGNN_MODEL_GCN: case FLOWGNN_MODEL_DGN: return 100;
        case FLOWGNN_MODEL_GAT: return 16;
        case FLOWGNN_MODEL_PNA: return 80;
        default: return -1;
    }
}

int flowgnn_create(int model, int device_id, flowgnn_engine** out) {
    if (!out) return FLOWGNN_ERR_ARG;
    *out = nullptr;
    Model* m = nullptr;
    switch (model) {
        case FLOWGNN_MODEL_GIN: m = make_gin_model(false); break;
        case FLOWGNN_MODEL_GIN_VN: m = make_gin_model(true); break;
        case FLOWGNN_MODEL_GCN: m = make_gcn_model(); break;
        case FLOWGNN_MODEL_PNA: m = make_pna_model(); break;
        case FLOWGNN_MODEL_DGN: m = make_dgn_model(); break;
        case FLOWGNN_MODEL_GAT: m = make_gat_model(); break;
        default: return FLOWGNN_ERR_UNSUPPORTED;
    }
    flowgnn_engine* e = new flowgnn_engine();
    e->model_id = model;
    e->device = device_id;
    e->model = m;
    e->emb_dim = flowgnn_embedding_dim(model);  // (the embeddings' width: GAT's rows in HBM, Model::emb_dim(), are its four heads side by side)
    e->graph_mode = e->opts.i("hipgraph");
    m->configure(e->opts);
    int rc = use_device(e);
    if (!rc) {
        hipError_t he = hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking);
        e->stream = e->own_stream;
        // Copies on a stream of their own, at the highest priority (priorities have their own hardware queues): through the null stream
        // a copy can share a queue with ANOTHER engine's kernels -- which queue a stream lands on depends on how many streams the
        // process has had -- and then waits for them: the entry points' copy / kernel pipeline ran at 31 ms instead of 13 in such runs.
        if (he == hipSuccess) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&e->copy_stream, hipStreamNonBlocking, hi) != hipSuccess) { (void)hipGetLastError(); e->copy_stream = nullptr; }
        }
        if (he == hipSuccess) he = hipMalloc((void**)&e->d_err, 2 * sizeof(int));  // [0] validation, [1] range flag
        if (he == hipSuccess) he = hipMemset(e->d_err, 0, 2 * sizeof(int));
        if (he != hipSuccess) {
            set_hip_error("engine init", he, __FILE__, __LINE__);
            rc = FLOWGNN_ERR_HIP;
        }
    }
    if (rc) {
        delete m;
        delete e;
        return rc;
    }
    *out = e;
    return FLOWGNN_OK;
}

int flowgnn_destroy(flowgnn_engine* e) {
    if (!e) return FLOWGNN_ERR_ARG;
    // best-effort teardown: nothing useful can be done with an error here
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    e->drop_graph();
    e->free_batch();
    for (const Output& o : kOutputs) (e->*o.slot).own.release();
    e->eig_plan.release();
    e->eig_io.release();
    e->ogb_vn.release();
    e->attn_pool.release();
    e->s2s.release();
    if (e->eig_done) (void)hipEventDestroy(e->eig_done);
    if (e->d_err) (void)hipFree(e->d_err);
    delete e->model;
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    delete e;
    return FLOWGNN_OK;
}

const char* flowgnn_last_error(const flowgnn_engine* e) {
    if (e && !e->err.empty()) return e->err.c_str();
    return fg::last_error_text();
}

int flowgnn_set_weights_gin(flowgnn_engine* e, const float* node_embedding_weight, const float* edge_embedding_weight,
                            const float* node_mlp_1_weights, const float* node_mlp_1_bias,
                            const float* node_mlp_2_weights, const float* node_mlp_2_bias,
                            const float* graph_pred_weights, const float* graph_pred_bias) {
    if (!e || (e->model_id != FLOWGNN_MODEL_GIN && e->model_id != FLOWGNN_MODEL_GIN_VN)) return FLOWGNN_ERR_ARG;
    const float* t[8] = {node_embedding_weight, edge_embedding_weight, node_mlp_1_weights, node_mlp_1_bias,
                         node_mlp_2_weights,    node_mlp_2_bias,       graph_pred_weights, graph_pred_bias};
    return flowgnn_set_weights(e, 8, t);
}

int flowgnn_set_weights(flowgnn_engine* e, int count, const float* const* tensors) {
    if (!e || !tensors || count != e->model->num_weight_tensors()) return FLOWGNN_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!tensors[i]) return FLOWGNN_ERR_ARG;
    ENGINE_TRY(e, begin_change(e));
    ENGINE_TRY(e, e->model->set_weights(tensors));
    return FLOWGNN_OK;
}

int flowgnn_load_weights_dir(flowgnn_engine* e, const char* dir) {
    if (!e || !dir) return FLOWGNN_ERR_ARG;
    ENGINE_TRY(e, begin_change(e));
    ENGINE_TRY(e, e->model->load_weights_dir(dir));
    return FLOWGNN_OK;
}

static int alloc_batch(flowgnn_engine* e, size_t G, size_t N, size_t E, bool attr, bool eig) {
    const int D = e->model->emb_dim(), SD = e->model->scratch_dim();
    G *= (size_t)e->num_tasks;  // capG counts result slots (only d_out and the small per-graph arrays scale with it)
    // (!d_nn: an engine's first batch may be an empty one -- a model without edge attributes would allocate nothing for it)
    if (G > e->capG || N > e->capN || E > e->capE || !e->d_nn || (attr && !e->d_ea) || (eig && !e->d_eig)) {
        // Capacities only grow, each on its own, and a regrow leaves an eighth of headroom: an engine that is handed the ranges of
        // a cut job one after the other (flowgnn_group_compute) sees counts that differ by a few percent from range to range, and
        // every reallocation is two dozen hipFree / hipMalloc pairs that wait for the device.
        const bool regrow = e->capN > 0 || e->capE > 0;
        if (G < e->capG) G = e->capG;
        if (N < e->capN) N = e->capN;
        if (E < e->capE) E = e->capE;
        if (regrow) { G += G / 8; N += N / 8; E += E / 8; }
        e->free_batch();
        const size_t g1 = G ? G : 1, n1 = N ? N : 1, e1 = E ? E : 1;
        // the four per-graph arrays share ONE allocation (d_nn is its base; flowgnn_set_batch places the other three behind it and
        // fills all four with one copy: every host -> device copy costs ~20 us whatever its size, which is what a dataset-sized
        // batch's flowgnn_set_batch is made of)
        EHIP_TRY(e, hipMalloc((void**)&e->d_nn, sizeof(int) * (4 * g1 + 2)));
        e->d_ne = e->d_noff = e->d_eoff = nullptr;
        EHIP_TRY(e, hipMalloc((void**)&e->d_nf, sizeof(int) * n1 * ND_FEATURE));
        EHIP_TRY(e, hipMalloc((void**)&e->d_el, sizeof(int) * e1 * 2));
        if (attr) EHIP_TRY(e, hipMalloc((void**)&e->d_ea, sizeof(int) * e1 * EDGE_ATTR));
        if (eig) EHIP_TRY(e, hipMalloc((void**)&e->d_eig, sizeof(float) * n1 * 4));
        EHIP_TRY(e, hipMalloc((void**)&e->d_rowptr, sizeof(int) * (n1 + 1)));
        EHIP_TRY(e, hipMalloc((void**)&e->d_src, sizeof(int) * e1));
        EHIP_TRY(e, hipMalloc((void**)&e->d_eid, sizeof(int) * e1));
        EHIP_TRY(e, hipMalloc((void**)&e->d_ecode, sizeof(uint8_t) * e1));
        EHIP_TRY(e, hipMalloc((void**)&e->d_outdeg, sizeof(int) * n1));
        EHIP_TRY(e, hipMalloc((void**)&e->d_gsrc, sizeof(int) * e1));
        EHIP_TRY(e, hipMalloc((void**)&e->d_gdst, sizeof(int) * e1));
        EHIP_TRY(e, hipMalloc((void**)&e->d_cursor, sizeof(int) * n1));
        EHIP_TRY(e, hipMalloc((void**)&e->d_tmp, sizeof(int) * e1 * 2));
        EHIP_TRY(e, hipMalloc((void**)&e->d_bsums, sizeof(int) * (n1 / 2048 + 2)));
        // + 4 KiB slack: tile loaders read whole 1 KiB pieces and may run past the last row
        EHIP_TRY(e, hipMalloc((void**)&e->d_h0, sizeof(float) * n1 * D + 4096));
        EHIP_TRY(e, hipMalloc((void**)&e->d_h1, sizeof(float) * n1 * D + 4096));
        EHIP_TRY(e, hipMalloc((void**)&e->d_scratch, sizeof(float) * n1 * (SD > 0 ? SD : 1) + 4096));
        EHIP_TRY(e, hipMalloc((void**)&e->d_out, sizeof(float) * g1));
        e->capG = G; e->capN = N; e->capE = E;
    }
    return 0;
}

int flowgnn_set_job_totals(flowgnn_engine* e, long long job_nodes, long long job_edges) {
    if (!e) return FLOWGNN_ERR_ARG;
    if ((job_nodes < 0) != (job_edges < 0)) {
        e->err = "flowgnn_set_job_totals: both totals, or -1 for both";
        fg::set_last_error(e->err.c_str());
        return FLOWGNN_ERR_ARG;
    }
    e->job_n = job_nodes < 0 ? -1 : job_nodes;
    e->job_e = job_edges < 0 ? -1 : job_edges;
    return FLOWGNN_OK;
}

int flowgnn_set_job_tile_fill(flowgnn_engine* e, double fill) {
    if (!e) return FLOWGNN_ERR_ARG;
    e->job_fill = fill < 0.0 ? -1.0 : fill;
    return FLOWGNN_OK;
}

int flowgnn_graph_tile_fill(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, double* fill) {
    if (!e || !fill || num_graphs < 0 || (num_graphs > 0 && (!nums_of_nodes || !nums_of_edges))) return FLOWGNN_ERR_ARG;
    *fill = graph_tile_fill(e->model, num_graphs, nums_of_nodes, nums_of_edges);
    return FLOWGNN_OK;
}

// per-graph counts of a batch and what the host derives from them: prefix sums, totals, largest graph (the limit checks of
// flowgnn_set_batch, shared by flowgnn_set_batch_device)
struct BatchCounts {
    std::vector<int> noff, eoff;  // [G + 1]
    long long N = 0, E = 0;
    int mx_n = 0, mx_e = 0;
};
static int batch_counts(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, BatchCounts* c) {
    if (!e || num_graphs < 0) return FLOWGNN_ERR_ARG;
    if (num_graphs > 0 && (!nums_of_nodes || !nums_of_edges)) return FLOWGNN_ERR_ARG;
    // prefix sums of node / edge counts: what the reference carries as nodes_offset / edges_offset
    // (GIN/src/GIN_compute.cc:44,96-97)
    std::vector<int>& noff = c->noff;
    std::vector<int>& eoff = c->eoff;
    noff.assign((size_t)num_graphs + 1, 0);
    eoff.assign((size_t)num_graphs + 1, 0);
    long long N = 0, E = 0;
    int mx_n = 0, mx_e = 0;
    for (int g = 0; g < num_graphs; g++) {
        if (nums_of_nodes[g] <= 0 || nums_of_edges[g] < 0) {
            e->err = "graph with num_of_nodes <= 0 or num_of_edges < 0";
            return FLOWGNN_ERR_ARG;
        }
        noff[g] = (int)N;
        eoff[g] = (int)E;
        if (nums_of_nodes[g] > mx_n) mx_n = nums_of_nodes[g];
        if (nums_of_edges[g] > mx_e) mx_e = nums_of_edges[g];
        N += nums_of_nodes[g];
        E += nums_of_edges[g];
        if (N > 0x7fffffffLL / 128 || E > 0x7fffffffLL / 4) {
            e->err = "batch too large for int32 indexing";
            return FLOWGNN_ERR_ARG;
        }
    }
    noff[num_graphs] = (int)N;
    eoff[num_graphs] = (int)E;
    c->N = N; c->E = E; c->mx_n = mx_n; c->mx_e = mx_e;
    return FLOWGNN_OK;
}

// a synchronous host -> device copy on the engine's copy queue (the source is the caller's pageable memory: the call returns when
// the data has left it)
static int h2d_sync(flowgnn_engine* e, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return 0;
    if (e->copy_stream) {
        EHIP_TRY(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->copy_stream));
        EHIP_TRY(e, hipStreamSynchronize(e->copy_stream));
    } else {
        EHIP_TRY(e, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    }
    return 0;
}
// ... and device -> host (on the engine's own copy queue: the null stream may share a hardware queue with another engine's kernels)
static int d2h_sync(flowgnn_engine* e, void* dst, const void* src, size_t bytes, const char* what) {
    hipError_t he = e->copy_stream ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->copy_stream) : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    if (he == hipSuccess && e->copy_stream) he = hipStreamSynchronize(e->copy_stream);
    return he == hipSuccess ? 0 : EHIP_FAIL(e, what, he);
}

// the bulk arrays of flowgnn_set_batch, host -> d_nf / d_el / d_ea / d_eig.
// copy_mu (flowgnn_group_compute): held around the large host -> device copies only -- one copier per DEVICE at a time, while another
// engine of the same device packs its next range on the host or packs its tiles
static int upload_host_arrays(flowgnn_engine* e, const BatchCounts& c, const int* node_feature, const int* edge_list, const int* edge_attr,
                              const float* node_eigen, std::mutex* copy_mu) {
    const bool attr = e->model->has_edge_attr();
    const bool eig = (e->model_id == FLOWGNN_MODEL_DGN);
    const long long N = c.N, E = c.E;
    // The three int32 arrays narrowed on the host (9 B per node, 5 B per edge: a quarter of the bytes), copied from pinned memory and
    // widened again on the GPU (h2d_pack.cpp; option h2d_pack, 0 = off).  Large batches only: below a few megabytes the plain copies
    // are latency, not bytes.  Not for GAT (its nine node features are NUMBERS, any integer is valid input) nor for graphs whose
    // node ids do not fit 16 bits.
    const size_t plain_bytes = sizeof(int) * ((size_t)N * ND_FEATURE + (size_t)E * 2 + (attr ? (size_t)E * EDGE_ATTR : 0));
    const int pack_threads = e->opts.i("h2d_pack") > 0 ? host_threads(e->opts.i("h2d_pack")) : 0;
    if (pack_threads > 0 && e->copy_stream && plain_bytes >= ((size_t)8 << 20) && c.mx_n <= 65535 && e->model_id != FLOWGNN_MODEL_GAT) {
        size_t off_e = 0, off_a = 0;
        const size_t pb = fg::h2d_pack_bytes((size_t)N, (size_t)E, attr, &off_e, &off_a);
        EHIP_TRY(e, e->h_pack.reserve(pb, true));  // (an eighth of headroom: the ranges of a cut job differ by a few percent)
        EHIP_TRY(e, e->d_pack.reserve(pb, true));
        uint8_t* const h_pack = (uint8_t*)e->h_pack.p;
        const uint8_t* const d_pack = (const uint8_t*)e->d_pack.p;
        fg::h2d_pack(node_feature, edge_list, attr ? edge_attr : nullptr, (size_t)N, (size_t)E, h_pack, pack_threads);
        std::unique_lock<std::mutex> lk;
        if (copy_mu) lk = std::unique_lock<std::mutex>(*copy_mu);
        EHIP_TRY(e, hipMemcpyAsync(e->d_pack.p, h_pack, pb, hipMemcpyHostToDevice, e->copy_stream));
        launch_unpack_batch(d_pack, d_pack + off_e, attr ? d_pack + off_a : nullptr, e->d_nf, e->d_el, attr ? e->d_ea : nullptr,
                            (long long)N, (long long)E, e->copy_stream);
        if (eig) EHIP_TRY(e, hipMemcpyAsync(e->d_eig, node_eigen, sizeof(float) * (size_t)N * 4, hipMemcpyHostToDevice, e->copy_stream));
        EHIP_TRY(e, hipStreamSynchronize(e->copy_stream));
    } else {
        std::unique_lock<std::mutex> lk;
        if (copy_mu) lk = std::unique_lock<std::mutex>(*copy_mu);
        ENGINE_TRY(e, h2d_sync(e, e->d_nf, node_feature, sizeof(int) * (size_t)N * ND_FEATURE));
        ENGINE_TRY(e, h2d_sync(e, e->d_el, edge_list, sizeof(int) * (size_t)E * 2));
        if (attr) ENGINE_TRY(e, h2d_sync(e, e->d_ea, edge_attr, sizeof(int) * (size_t)E * EDGE_ATTR));
        if (eig) ENGINE_TRY(e, h2d_sync(e, e->d_eig, node_eigen, sizeof(float) * (size_t)N * 4));
    }
    return 0;
}

// several host vectors as ONE allocation and one copy, in the order given: the first vector takes the others behind it
static int upload_concat(flowgnn_engine* e, fg::GrowBuf& buf, bool headroom, std::vector<int>& first, std::initializer_list<const std::vector<int>*> rest) {
    for (const std::vector<int>* v : rest) first.insert(first.end(), v->begin(), v->end());
    EHIP_TRY(e, buf.reserve(sizeof(int) * first.size(), headroom));
    return h2d_sync(e, buf.p, first.data(), sizeof(int) * first.size());
}

// The batch state both set_batch entry points build from the per-graph counts: buffers, counts and offsets on the device, graph
// tiles, bin-packed tiles, job totals and fill.  `upload` fills d_nf / d_el / d_ea / d_eig, synchronously, where flowgnn_set_batch
// always copied them (after the buffers, before the tiles); nullptr: the caller enqueues that transfer itself once this returns
// (flowgnn_set_batch_device: after the reset of the error word, so that what its ingest reports survives until the next batch).
static int set_batch_state(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, const BatchCounts& c,
                           const std::function<int()>& upload) {
    const bool attr = e->model->has_edge_attr();
    const bool eig = (e->model_id == FLOWGNN_MODEL_DGN);
    const long long N = c.N, E = c.E;
    const int mx_n = c.mx_n, mx_e = c.mx_e;

    ENGINE_TRY(e, begin_change(e));
    e->batch_ready = false;
    e->ran = false;
    ENGINE_TRY(e, alloc_batch(e, (size_t)num_graphs, (size_t)N, (size_t)E, attr, eig));
    {   // counts and offsets: one staging vector, one copy
        const size_t G = (size_t)num_graphs;
        std::vector<int> meta(4 * G + 2);
        if (G) { memcpy(meta.data(), nums_of_nodes, sizeof(int) * G); memcpy(meta.data() + G, nums_of_edges, sizeof(int) * G); }
        memcpy(meta.data() + 2 * G, c.noff.data(), sizeof(int) * (G + 1));
        memcpy(meta.data() + 3 * G + 1, c.eoff.data(), sizeof(int) * (G + 1));
        e->d_ne = e->d_nn + G; e->d_noff = e->d_nn + 2 * G; e->d_eoff = e->d_nn + 3 * G + 1;
        ENGINE_TRY(e, h2d_sync(e, e->d_nn, meta.data(), sizeof(int) * meta.size()));
    }
    if (upload) ENGINE_TRY(e, upload());

    // graph-aligned tiles for kernels that keep whole graphs on chip across layers (GraphTiles, common.h), planned on the host
    // (tile_pack.cpp) AFTER the bulk upload: under flowgnn_group_compute one engine plans while the other copies
    fg::TileLimits lim;
    e->model->graph_tile_limits(lim.rows, lim.edges);
    e->model->sub_tile_limits(lim.sub_rows, lim.sub_edges);
    lim.balance = e->opts.on("tile_balance");
    lim.binpack = e->model->wants_packed_tile_lists();
    lim.threads = e->opts.i("h2d_pack") > 0 ? host_threads(e->opts.i("h2d_pack")) : 1;
    fg::TilePlan plan;
    fg::plan_tiles(lim, num_graphs, nums_of_nodes, nums_of_edges, &plan);
    GraphTiles& gt = e->db.gtiles;
    gt = GraphTiles{};
    if (plan.ok) {
        const size_t T1 = plan.row_start.size();
        ENGINE_TRY(e, upload_concat(e, e->tiles, true, plan.row_start, {&plan.graph_start}));  // headroom: ranges of a cut job differ by a few tiles
        gt.row_start = (const int*)e->tiles.p; gt.graph_start = gt.row_start + T1;
        gt.n_tiles = (int)T1 - 1; gt.rows = lim.rows; gt.edges = lim.edges; gt.ok = true;
        // a shard that was told the fill of its JOB (flowgnn_set_job_tile_fill; the group and the entry points do) takes the job's side
        // of the models' thresholds whatever its own graphs pack to
        gt.fill = e->job_fill >= 0.0 ? e->job_fill : plan.fill;
    }
    if (!plan.bp_list.empty()) {
        const size_t T1 = plan.bp_graph.size();
        ENGINE_TRY(e, upload_concat(e, e->bp, true, plan.bp_list, {&plan.bp_lrow, &plan.bp_graph, &plan.bp_row}));  // headroom, as above
        gt.bp_list = (const int*)e->bp.p;
        gt.bp_lrow = gt.bp_list + num_graphs;
        gt.bp_graph = gt.bp_list + 2 * (size_t)num_graphs;
        gt.bp_row = gt.bp_graph + T1;
        gt.bp_tiles = (int)T1 - 1;
    }
    if (plan.sub_ok) {
        const size_t n_sub4 = plan.sub.size(), n_big2 = plan.big_row.size();
        ENGINE_TRY(e, upload_concat(e, e->sub, false, plan.sub, {&plan.big_row, &plan.big_graph}));  // no headroom (a development-only path)
        gt.sub = (const int*)e->sub.p; gt.n_sub = (int)(n_sub4 / 4); gt.sub_rows = lim.sub_rows; gt.sub_edges = lim.sub_edges;
        gt.big_row = gt.sub + n_sub4; gt.big_graph = gt.big_row + n_big2; gt.n_big = (int)(n_big2 / 2);
        gt.sub_ok = true;
        gt.sub_fill = plan.sub_fill;
    }

    e->G = num_graphs; e->N = N; e->E = E;
    e->max_nodes = mx_n; e->max_edges = mx_e;
    e->has_attr = attr; e->has_eig = eig;
    DeviceBatch& db = e->db;
    db.b.num_graphs = num_graphs; db.b.n_tot = (int)N; db.b.e_tot = (int)E;
    db.job_n = e->job_n >= 0 ? std::max(e->job_n, N) : N;
    db.job_e = e->job_e >= 0 ? std::max(e->job_e, E) : E;
    db.b.nums_of_nodes = e->d_nn; db.b.nums_of_edges = e->d_ne;
    db.b.node_off = e->d_noff; db.b.edge_off = e->d_eoff;
    db.b.node_feature = e->d_nf; db.b.edge_list = e->d_el; db.b.edge_attr = attr ? e->d_ea : nullptr;
    db.csr.row_ptr = e->d_rowptr; db.csr.src = e->d_src; db.csr.eid = e->d_eid;
    db.csr.ecode = e->d_ecode; db.csr.out_deg = e->d_outdeg;
    db.csr.gsrc = e->d_gsrc; db.csr.gdst = e->d_gdst; db.csr.cursor = e->d_cursor; db.csr.tmp = e->d_tmp;
    db.csr.block_sums = e->d_bsums; db.csr.err = e->d_err;
    db.node_eigen = eig ? e->d_eig : nullptr;
    db.h[0] = e->d_h0; db.h[1] = e->d_h1; db.scratch = e->d_scratch; db.out = e->d_out;
    db.num_tasks = e->num_tasks;
    db.pooling = e->pooling;
    db.gin_eps_on = e->gin_eps_on;
    for (int l = 0; l < FLOWGNN_MAX_NUM_LAYERS; l++) db.gin_self_scale[l] = (float)(1.0f + e->gin_eps[l]);
    db.ogb_vn = e->ogb_vn_on ? (const float*)e->ogb_vn.p : nullptr;
    db.attn_pool = e->attn_pool_on ? e->attn_pool.p : nullptr;
    db.s2s = e->s2s_steps ? e->s2s.p : nullptr;
    db.s2s_steps = e->s2s_steps;
    db.jk = e->jk;
    db.residual = e->residual;
    db.final_h = 0;
    db.tap = nullptr;
    db.tap_dim = 0;
    db.csr_built = false;
    db.max_nodes = mx_n; db.max_edges = mx_e;
    EHIP_TRY(e, hipMemset(e->d_err, 0, 2 * sizeof(int)));
    e->db.range_flag = e->d_err + 1;
    e->force_exact = false;
    e->batch_ready = true;
    for (const Output& o : kOutputs) (e->*o.slot).user = (e->*o.slot).last = nullptr;
    e->attn_mask_last = 0;
    for (const Output& o : kOutputs)
        if (int rc = place(e, o)) return rc;
    e->db.attn_mask = e->attn_mask;
    return FLOWGNN_OK;
}

}  // extern "C"

// fill of the model's graph tiles when `num_graphs` graphs are packed greedily in order (the packing flowgnn_set_batch does), without
// the last tile; 1 for a one-tile batch, 0 when a graph exceeds the tile limits (no resident path), -1 when the model has no tiles
double graph_tile_fill(fg::Model* model, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges) {
    int t_rows = 0, t_edges = 0;
    model->graph_tile_limits(t_rows, t_edges);
    if (t_rows <= 0 || num_graphs <= 0) return -1.0;
    return fg::greedy_tile_fill(t_rows, t_edges, num_graphs, nums_of_nodes, nums_of_edges);
}

// flowgnn_set_batch (and the group's ranges, group.hip): host arrays
int set_batch_impl(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, const int* node_feature,
                   const int* edge_list, const int* edge_attr, const float* node_eigen, std::mutex* copy_mu) {
    BatchCounts c;
    const int rc = batch_counts(e, num_graphs, nums_of_nodes, nums_of_edges, &c);
    if (rc) return rc;
    const bool attr = e->model->has_edge_attr();
    const bool eig = (e->model_id == FLOWGNN_MODEL_DGN);
    if (c.N > 0 && !node_feature) return FLOWGNN_ERR_ARG;
    if (c.E > 0 && (!edge_list || (attr && !edge_attr))) return FLOWGNN_ERR_ARG;
    if (eig && c.N > 0 && !node_eigen) return FLOWGNN_ERR_ARG;
    return set_batch_state(e, num_graphs, nums_of_nodes, nums_of_edges, c,
                           [&]() { return upload_host_arrays(e, c, node_feature, edge_list, edge_attr, node_eigen, copy_mu); });
}

extern "C" {

int flowgnn_set_batch(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                      const int* node_feature, const int* edge_list, const int* edge_attr, const float* node_eigen) {
    return set_batch_impl(e, num_graphs, nums_of_nodes, nums_of_edges, node_feature, edge_list, edge_attr, node_eigen, nullptr);
}

// flowgnn_set_batch_device's guard: a non-empty array must be memory of the engine's device, and the bytes the counts imply must lie
// inside its allocation (with XNACK off, a kernel that reads pageable host memory or runs past an allocation faults the device)
static int check_device_array(const flowgnn_engine* e, const void* p, size_t bytes, const char* what, const char* api = "flowgnn_set_batch_device") {
    if (!p || bytes == 0) return 0;
    char msg[256];
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(msg, sizeof(msg), "%s: %s is not memory the HIP runtime knows (pageable host memory?)", api, what);
        fg::set_last_error(msg);  // (ENGINE_TRY hands it to the engine)
        return FLOWGNN_ERR_ARG;
    }
    if (a.type != hipMemoryTypeDevice || a.device != e->device) {
        snprintf(msg, sizeof(msg), "%s: %s is not device memory of device %d (memory type %d, device %d)", api, what,
                 e->device, (int)a.type, a.device);
        fg::set_last_error(msg);  // (ENGINE_TRY hands it to the engine)
        return FLOWGNN_ERR_ARG;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(msg, sizeof(msg), "%s: no allocation range for %s", api, what);
        fg::set_last_error(msg);  // (ENGINE_TRY hands it to the engine)
        return FLOWGNN_ERR_ARG;
    }
    const uintptr_t lo = (uintptr_t)p, end = (uintptr_t)base + size;
    if (lo < (uintptr_t)base || bytes > end - lo) {
        snprintf(msg, sizeof(msg), "%s: %s holds %zu bytes from this pointer to the end of its allocation, the counts imply %zu",
                 api, what, (size_t)(end > lo ? end - lo : 0), bytes);
        fg::set_last_error(msg);  // (ENGINE_TRY hands it to the engine)
        return FLOWGNN_ERR_ARG;
    }
    return 0;
}

int flowgnn_set_batch_device(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, int layout,
                             const void* node_feature, const void* edge_list, const void* edge_attr, const float* node_eigen) {
    BatchCounts c;
    int rc = batch_counts(e, num_graphs, nums_of_nodes, nums_of_edges, &c);
    if (rc) return rc;
    if (layout != FLOWGNN_LAYOUT_REFERENCE && layout != FLOWGNN_LAYOUT_PYG) {
        e->err = "flowgnn_set_batch_device: unknown layout";
        return FLOWGNN_ERR_ARG;
    }
    const bool attr = e->model->has_edge_attr();
    const bool eig = (e->model_id == FLOWGNN_MODEL_DGN);
    const size_t N = (size_t)c.N, E = (size_t)c.E;
    if ((N > 0 && !node_feature) || (E > 0 && (!edge_list || (attr && !edge_attr))) || (eig && N > 0 && !node_eigen)) {
        e->err = "flowgnn_set_batch_device: an array the model needs is NULL";
        return FLOWGNN_ERR_ARG;
    }
    // the guard, before anything is enqueued (every non-null array, whether the model reads it or not)
    const size_t w = layout == FLOWGNN_LAYOUT_PYG ? sizeof(long long) : sizeof(int);
    ENGINE_TRY(e, use_device(e));
    ENGINE_TRY(e, check_device_array(e, node_feature, w * N * ND_FEATURE, "node_feature"));
    ENGINE_TRY(e, check_device_array(e, edge_list, w * E * 2, "edge_list"));
    ENGINE_TRY(e, check_device_array(e, edge_attr, w * E * EDGE_ATTR, "edge_attr"));
    ENGINE_TRY(e, check_device_array(e, node_eigen, sizeof(float) * N * 4, "node_eigen"));
    rc = set_batch_state(e, num_graphs, nums_of_nodes, nums_of_edges, c, nullptr);
    if (rc) return rc;
    // the ingest, on the launch stream: ordered after the caller's work on it, before the next flowgnn_run; nothing waits for it
    {
        ProfScope p(e->prof, "ingest", e->stream);
        hipError_t he = hipSuccess;
        if (layout == FLOWGNN_LAYOUT_PYG) {
            fg::launch_ingest_pyg((const long long*)node_feature, (const long long*)edge_list, attr ? (const long long*)edge_attr : nullptr,
                                  e->d_nf, e->d_el, attr ? e->d_ea : nullptr, e->d_noff, e->d_eoff, num_graphs, c.N, c.E, e->d_err,
                                  e->model_id == FLOWGNN_MODEL_GAT ? ERR_NODE_FEAT : 0, e->device, e->stream);
            he = hipGetLastError();
        } else {
            if (N) he = hipMemcpyAsync(e->d_nf, node_feature, sizeof(int) * N * ND_FEATURE, hipMemcpyDeviceToDevice, e->stream);
            if (he == hipSuccess && E) he = hipMemcpyAsync(e->d_el, edge_list, sizeof(int) * E * 2, hipMemcpyDeviceToDevice, e->stream);
            if (he == hipSuccess && E && attr)
                he = hipMemcpyAsync(e->d_ea, edge_attr, sizeof(int) * E * EDGE_ATTR, hipMemcpyDeviceToDevice, e->stream);
        }
        if (he == hipSuccess && eig && N) he = hipMemcpyAsync(e->d_eig, node_eigen, sizeof(float) * N * 4, hipMemcpyDeviceToDevice, e->stream);
        if (he != hipSuccess) {
            e->batch_ready = false;
            return EHIP_FAIL(e, "flowgnn_set_batch_device: ingest", he);
        }
    }
    return FLOWGNN_OK;
}

// ---- flowgnn_laplacian_eigen*: DGN's node_eigen from the graphs alone (kernels: eigen.hip).  Nothing of the resident batch, the
// recorded launch sequence or the output slots is touched: the engine lends its device, its launch stream and scratch of its own.
// The plan both functions share: counts -> offsets and the three size-class lists, one upload, one launch per non-empty class.
static int laplacian_eigen_classes(flowgnn_engine* e, const char* api, int num_graphs, const int* nums_of_nodes, std::vector<int> (&cls)[3]) {
    for (int g = 0; g < num_graphs; g++) {
        const int n = nums_of_nodes[g];
        if (n > FLOWGNN_EIGEN_MAX_NODES) {
            char msg[160];
            snprintf(msg, sizeof(msg), "%s: graph %d has %d nodes, the eigensolver takes up to %d", api, g, n, FLOWGNN_EIGEN_MAX_NODES);
            e->err = msg;
            return FLOWGNN_ERR_UNSUPPORTED;
        }
        cls[n <= 32 ? 0 : n <= 64 ? 1 : 2].push_back(g);
    }
    return FLOWGNN_OK;
}
static int laplacian_eigen_launch(flowgnn_engine* e, const char* api, const std::vector<int> (&cls)[3], const BatchCounts& c, bool pyg,
                                  const void* d_edges, float* d_out) {
    // the previous call's kernels read eig_plan: wait for them before it is rewritten (or regrown)
    if (e->eig_done) EHIP_TRY(e, hipEventSynchronize(e->eig_done));
    else EHIP_TRY(e, hipEventCreateWithFlags(&e->eig_done, hipEventDisableTiming));
    std::vector<int> plan(c.noff);
    const size_t at_eoff = plan.size(), at_list = at_eoff + c.eoff.size();
    ENGINE_TRY(e, upload_concat(e, e->eig_plan, true, plan, {&c.eoff, &cls[0], &cls[1], &cls[2]}));
    const int* const d_plan = (const int*)e->eig_plan.p;
    size_t at = at_list;
    for (int k = 0; k < 3; k++) {
        fg::launch_laplacian_eigen(k, d_plan + at, (int)cls[k].size(), d_plan, d_plan + at_eoff, d_edges, c.E, pyg, d_out, e->stream);
        at += cls[k].size();
    }
    const hipError_t he = hipGetLastError();
    if (he != hipSuccess) return EHIP_FAIL(e, api, he);
    EHIP_TRY(e, hipEventRecord(e->eig_done, e->stream));
    return FLOWGNN_OK;
}

int flowgnn_laplacian_eigen_max_nodes(void) { return FLOWGNN_EIGEN_MAX_NODES; }

int flowgnn_laplacian_eigen_device(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, int layout,
                                   const void* edge_list, float* node_eigen) {
    static const char* const api = "flowgnn_laplacian_eigen_device";
    BatchCounts c;
    const int rc = batch_counts(e, num_graphs, nums_of_nodes, nums_of_edges, &c);
    if (rc) return rc;
    if (layout != FLOWGNN_LAYOUT_REFERENCE && layout != FLOWGNN_LAYOUT_PYG) {
        e->err = "flowgnn_laplacian_eigen_device: unknown layout";
        return FLOWGNN_ERR_ARG;
    }
    if (num_graphs == 0) return FLOWGNN_OK;
    const size_t N = (size_t)c.N, E = (size_t)c.E;
    if (!node_eigen || (E > 0 && !edge_list)) {
        e->err = "flowgnn_laplacian_eigen_device: edge_list or node_eigen is NULL";
        return FLOWGNN_ERR_ARG;
    }
    const size_t w = layout == FLOWGNN_LAYOUT_PYG ? sizeof(long long) : sizeof(int);
    ENGINE_TRY(e, use_device(e));
    ENGINE_TRY(e, check_device_array(e, edge_list, w * E * 2, "edge_list", api));
    ENGINE_TRY(e, check_device_array(e, node_eigen, sizeof(float) * N * 4, "node_eigen", api));
    std::vector<int> cls[3];
    if (const int crc = laplacian_eigen_classes(e, api, num_graphs, nums_of_nodes, cls)) return crc;
    return laplacian_eigen_launch(e, api, cls, c, layout == FLOWGNN_LAYOUT_PYG, edge_list, node_eigen);
}

int flowgnn_laplacian_eigen(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, const int* edge_list,
                            float* node_eigen) {
    static const char* const api = "flowgnn_laplacian_eigen";
    BatchCounts c;
    const int rc = batch_counts(e, num_graphs, nums_of_nodes, nums_of_edges, &c);
    if (rc) return rc;
    if (num_graphs == 0) return FLOWGNN_OK;
    const size_t N = (size_t)c.N, E = (size_t)c.E;
    if (!node_eigen || (E > 0 && !edge_list)) {
        e->err = "flowgnn_laplacian_eigen: edge_list or node_eigen is NULL";
        return FLOWGNN_ERR_ARG;
    }
    std::vector<int> cls[3];
    if (const int crc = laplacian_eigen_classes(e, api, num_graphs, nums_of_nodes, cls)) return crc;
    for (int g = 0; g < num_graphs; g++) {
        const int n = nums_of_nodes[g];
        for (int i = c.eoff[g]; i < c.eoff[g + 1]; i++) {
            const int u = edge_list[2 * (size_t)i], v = edge_list[2 * (size_t)i + 1];
            if (u < 0 || u >= n || v < 0 || v >= n) {
                char msg[160];
                snprintf(msg, sizeof(msg), "%s: edge %d of graph %d is (%d, %d), the graph has %d nodes", api, i - c.eoff[g], g, u, v, n);
                e->err = msg;
                return FLOWGNN_ERR_EDGE_RANGE;
            }
        }
    }
    ENGINE_TRY(e, use_device(e));
    if (e->eig_done) EHIP_TRY(e, hipEventSynchronize(e->eig_done));  // (eig_io may be regrown: nothing reads it any more)
    const size_t edge_bytes = (sizeof(int) * E * 2 + 15) / 16 * 16;
    EHIP_TRY(e, e->eig_io.reserve(edge_bytes + sizeof(float) * N * 4, true));
    float* const d_out = (float*)((char*)e->eig_io.p + edge_bytes);
    ENGINE_TRY(e, h2d_sync(e, e->eig_io.p, edge_list, sizeof(int) * E * 2));
    if (const int lrc = laplacian_eigen_launch(e, api, cls, c, false, e->eig_io.p, d_out)) return lrc;
    EHIP_TRY(e, hipStreamSynchronize(e->stream));
    return d2h_sync(e, node_eigen, d_out, sizeof(float) * N * 4, api);
}

int flowgnn_run(flowgnn_engine* e) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (!e->batch_ready || !e->model->weights_ready()) {
        e->err = "flowgnn_run: weights or batch not set";
        return FLOWGNN_ERR_STATE;
    }
    ENGINE_TRY(e, use_device(e));
    for (const Output& o : kOutputs) (e->*o.slot).last = e->db.*o.field;
    e->attn_mask_last = e->db.attn_mask;
    if (e->G == 0) { e->ran = true; return FLOWGNN_OK; }
    const bool want_graph = e->graph_mode != 0 && !e->prof.enabled && (e->graph_mode > 1 || e->N <= (1ll << 20));
    if (want_graph && e->graph_ok) {
        e->db.tap = e->graph_tap;
        e->db.tap_dim = e->graph_tap_dim;
        e->db.final_h = e->graph_final_h;
        e->db.h_valid = e->graph_h_valid;
        EHIP_TRY(e, hipGraphLaunch(e->gexec, e->stream));
        e->graph_replays++;
        e->ran = true;
        return FLOWGNN_OK;
    }
    const bool capture = want_graph && e->plain_runs >= 1;
    if (capture) {
        hipError_t hc = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
        if (hc != hipSuccess) {
            (void)hipGetLastError();
            e->graph_mode = 0;  // this runtime cannot capture: stay on plain launches
            return flowgnn_run(e);
        }
    }
    int frc = FLOWGNN_OK;
    e->db.tap = nullptr;
    e->db.tap_dim = 0;
    e->db.h_valid = true;
    e->model->set_exact(e->force_exact);
    frc = engine_forward(e);
    if (capture) {
        hipGraph_t g = nullptr;
        hipError_t hc = hipStreamEndCapture(e->stream, &g);
        if (hc == hipSuccess && frc == FLOWGNN_OK && g) hc = hipGraphInstantiate(&e->gexec, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
        if (hc != hipSuccess || frc != FLOWGNN_OK || !e->gexec) {
            (void)hipGetLastError();
            e->drop_graph();
            e->graph_mode = 0;  // something in this model's forward is not capturable: plain launches from now on
            return flowgnn_run(e);
        }
        e->graph_ok = true;
        e->graph_h_valid = e->db.h_valid;
        e->graph_tap = e->db.tap;
        e->graph_tap_dim = e->db.tap_dim;
        e->graph_final_h = e->db.final_h;
        EHIP_TRY(e, hipGraphLaunch(e->gexec, e->stream));  // the capture only recorded: this is the run itself
        e->graph_replays++;
        e->ran = true;
        return FLOWGNN_OK;
    }
    if (frc != FLOWGNN_OK) {
        e->err = fg::last_error_text();
        return frc;
    }
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) return EHIP_FAIL(e, "kernel launch", he);
    e->plain_runs++;
    e->ran = true;
    return FLOWGNN_OK;
}

int flowgnn_sync(flowgnn_engine* e) {
    if (!e) return FLOWGNN_ERR_ARG;
    ENGINE_TRY(e, use_device(e));
    hipError_t he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) return EHIP_FAIL(e, "hipStreamSynchronize", he);
    e->prof.collect();
    int flags[2] = {0, 0};
    if (int rc = d2h_sync(e, flags, e->d_err, sizeof(flags), "read error flag")) return rc;
    const int flag = flags[0];
    if (!flag && flags[1] && e->ran && !e->force_exact) {
        // an operand left the range in which the default kernels are fp32-accurate: repeat the pass on the exact
        // kernels, and keep this batch on them for later runs
        e->force_exact = true;
        e->exact_reruns++;
        e->drop_graph();  // the captured launches are the split-f16 ones
        EHIP_TRY(e, hipMemsetAsync(e->d_err + 1, 0, sizeof(int), e->stream));
        e->model->set_exact(true);
        int frc;
        {   // the repeated pass refills what the run filled: the logits, and every optional output where that run had it on
            KeepOutputFields keep(e->db);
            for (const Output& o : kOutputs) e->db.*o.field = (e->*o.slot).last;
            e->db.attn_mask = e->attn_mask_last;
            frc = engine_forward(e);
        }
        ENGINE_TRY(e, frc);
        he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) return EHIP_FAIL(e, "hipStreamSynchronize (exact re-run)", he);
        e->prof.collect();
    }
    if (flag) {
        e->err = flag == FLOWGNN_ERR_UNSUPPORTED
                     ? "a node of a graph beyond the per-graph size classes has more than 16384 in-edges (the index build's rank sort is quadratic per row)"
                     : "input validation failed on device (edge endpoint / edge attribute / node feature out of range)";
        return flag;
    }
    return FLOWGNN_OK;
}

int flowgnn_get_results(flowgnn_engine* e, float* out_host) {
    if (!e || (!out_host && e->G > 0)) return FLOWGNN_ERR_ARG;
    if (!e->ran) { e->err = "flowgnn_get_results before flowgnn_run"; return FLOWGNN_ERR_STATE; }
    int rc = flowgnn_sync(e);
    if (rc) return rc;
    if (e->G > 0) return d2h_sync(e, out_host, e->db.out, sizeof(float) * (size_t)e->G * e->num_tasks, "copy results");
    return FLOWGNN_OK;
}

int flowgnn_results_device(flowgnn_engine* e, void** d_out) {
    if (!e || !d_out) return FLOWGNN_ERR_ARG;
    if (!e->batch_ready) return FLOWGNN_ERR_STATE;
    *d_out = e->db.out;
    return FLOWGNN_OK;
}

int flowgnn_set_results_buffer(flowgnn_engine* e, void* device_ptr) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (!e->batch_ready) return FLOWGNN_ERR_STATE;
    // no device synchronisation: launches are stream-ordered, the pointer only matters to launches enqueued after this call
    // (a recorded launch sequence bakes the old pointer in, so that is dropped)
    if (e->gexec) { ENGINE_TRY(e, use_device(e)); e->drop_graph(); }
    e->db.out = device_ptr ? (float*)device_ptr : e->d_out;
    return FLOWGNN_OK;
}

// ---- the optional outputs (kOutputs): one helper per verb; each ABI function below is its own refusals, then the helper
static int switch_output(flowgnn_engine* e, const Output& o, int on) {
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();  // a recorded launch sequence is that of the other setting
    e->*o.on = on != 0;
    return place(e, o);
}

static int not_the_last_runs(flowgnn_engine* e, const Output& o, const char* api) {
    e->err = std::string(api) + ": the last flowgnn_run did not have " + o.noun + " on (" + o.setter + ")";
    return FLOWGNN_ERR_STATE;
}

// flowgnn_get_*: `count` elements (the batch's graphs, or nodes) are what makes a null out_host an error, and a copy worth making
static int get_output(flowgnn_engine* e, const Output& o, const char* api, float* out_host, long long flowgnn_engine::*count_of) {
    if (!e || (!out_host && e->*count_of > 0)) return FLOWGNN_ERR_ARG;
    const long long count = e->*count_of;
    const fg::OutSlot& s = e->*o.slot;
    if (!e->ran || (!s.last && e->G > 0) || (e->G == 0 && !is_on(e, o))) return not_the_last_runs(e, o, api);
    int rc = flowgnn_sync(e);
    if (rc) return rc;
    if (e->G > 0 && count > 0) return d2h_sync(e, out_host, s.last, sizeof(float) * o.floats(e), (std::string("copy ") + o.noun).c_str());
    return FLOWGNN_OK;
}

static int output_device(flowgnn_engine* e, const Output& o, const char* api, void** d_out) {
    if (!e || !d_out) return FLOWGNN_ERR_ARG;
    if (!e->ran || !(e->*o.slot).last) return not_the_last_runs(e, o, api);
    *d_out = (e->*o.slot).last;
    return FLOWGNN_OK;
}

// as flowgnn_set_results_buffer: no device synchronisation, the pointer matters to the launches enqueued after this call
static int begin_set_buffer(flowgnn_engine* e) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (!e->batch_ready) return FLOWGNN_ERR_STATE;
    ENGINE_TRY(e, use_device(e));
    if (e->gexec) e->drop_graph();
    return FLOWGNN_OK;
}
static int set_output_buffer(flowgnn_engine* e, const Output& o, void* device_ptr) {
    if (int rc = begin_set_buffer(e)) return rc;
    (e->*o.slot).user = (float*)device_ptr;
    return place(e, o);
}

int flowgnn_set_embeddings(flowgnn_engine* e, int on) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (on && e->numeric_mode == FLOWGNN_NUMERIC_Q6_10) {
        e->err = "flowgnn_set_embeddings: there are no fixed-point embeddings (FLOWGNN_NUMERIC_Q6_10)";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (on && e->s2s_steps) {
        e->err = "flowgnn_set_embeddings: the set2set pooling is on (flowgnn_set_set2set_pooling), and the vector its head reads is " +
                 std::to_string(2 * e->emb_dim) + " wide where every embeddings buffer is " + std::to_string(e->emb_dim) + " wide: there are no graph embeddings";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    return switch_output(e, kOutputs[OUT_EMB], on);
}

int flowgnn_get_embeddings(flowgnn_engine* e, float* out_host) { return get_output(e, kOutputs[OUT_EMB], "flowgnn_get_embeddings", out_host, &flowgnn_engine::G); }

int flowgnn_embeddings_device(flowgnn_engine* e, void** d_emb) { return output_device(e, kOutputs[OUT_EMB], "flowgnn_embeddings_device", d_emb); }

int flowgnn_set_embeddings_buffer(flowgnn_engine* e, void* device_ptr) { return set_output_buffer(e, kOutputs[OUT_EMB], device_ptr); }

int flowgnn_set_node_embeddings(flowgnn_engine* e, int on) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (on && e->numeric_mode == FLOWGNN_NUMERIC_Q6_10) {
        e->err = "flowgnn_set_node_embeddings: there are no fixed-point node embeddings (FLOWGNN_NUMERIC_Q6_10)";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    return switch_output(e, kOutputs[OUT_NEMB], on);
}

int flowgnn_get_node_embeddings(flowgnn_engine* e, float* out_host) { return get_output(e, kOutputs[OUT_NEMB], "flowgnn_get_node_embeddings", out_host, &flowgnn_engine::N); }

int flowgnn_node_embeddings_device(flowgnn_engine* e, void** d_rows) { return output_device(e, kOutputs[OUT_NEMB], "flowgnn_node_embeddings_device", d_rows); }

int flowgnn_set_node_embeddings_buffer(flowgnn_engine* e, void* device_ptr) { return set_output_buffer(e, kOutputs[OUT_NEMB], device_ptr); }

int flowgnn_set_node_logits(flowgnn_engine* e, int on) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (on && (e->model_id == FLOWGNN_MODEL_PNA || e->model_id == FLOWGNN_MODEL_DGN)) {
        e->err = "flowgnn_set_node_logits: PNA and DGN read the pooled vector through an MLP head, so a graph's logit is no mean of per-node terms";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (on && e->numeric_mode == FLOWGNN_NUMERIC_Q6_10) {
        e->err = "flowgnn_set_node_logits: there are no fixed-point node logits (FLOWGNN_NUMERIC_Q6_10)";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (on && e->pooling != FLOWGNN_POOL_MEAN) {
        e->err = "flowgnn_set_node_logits: the pooling is not the mean (flowgnn_set_pooling), and node logits are the terms whose mean is the logit";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (on && e->attn_pool_on) {
        e->err = "flowgnn_set_node_logits: the attention pooling is on (flowgnn_set_attention_pooling), and under it a graph's logit is no mean of per-node terms: there are no node logits";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (on && e->s2s_steps) {
        e->err = "flowgnn_set_node_logits: the set2set pooling is on (flowgnn_set_set2set_pooling), and under it a graph's logit is no mean of per-node terms: there are no node logits";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    return switch_output(e, kOutputs[OUT_NLOG], on);
}

int flowgnn_get_node_logits(flowgnn_engine* e, float* out_host) { return get_output(e, kOutputs[OUT_NLOG], "flowgnn_get_node_logits", out_host, &flowgnn_engine::N); }

int flowgnn_node_logits_device(flowgnn_engine* e, void** d_terms) { return output_device(e, kOutputs[OUT_NLOG], "flowgnn_node_logits_device", d_terms); }

int flowgnn_set_node_logits_buffer(flowgnn_engine* e, void* device_ptr) { return set_output_buffer(e, kOutputs[OUT_NLOG], device_ptr); }

int flowgnn_attention_shape(int model, int* layers, int* heads) {
    if (model != FLOWGNN_MODEL_GAT) {
        fg::set_last_error("flowgnn_attention_shape: only GAT has attention coefficients");
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (layers) *layers = 5;
    if (heads) *heads = 4;
    return FLOWGNN_OK;
}

int flowgnn_set_attention(flowgnn_engine* e, int layer_mask) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (layer_mask != 0 && e->model_id != FLOWGNN_MODEL_GAT) {
        e->err = "flowgnn_set_attention: only GAT has attention coefficients (the other models aggregate with fixed or degree-derived weights)";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    if (layer_mask < 0 || layer_mask > 31) {
        e->err = "flowgnn_set_attention: the layer mask has bits 0..4 (GAT's five layers), 0 = off";
        return FLOWGNN_ERR_ARG;
    }
    if (layer_mask && e->numeric_mode == FLOWGNN_NUMERIC_Q6_10) {
        e->err = "flowgnn_set_attention: there are no fixed-point attention coefficients (FLOWGNN_NUMERIC_Q6_10)";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();  // a recorded launch sequence is that of the other setting
    e->attn_mask = layer_mask;
    return place_attention(e);
}
}  // extern "C"

int get_attention_strided(flowgnn_engine* e, float* edge_host, size_t edge_stride, float* self_host, size_t self_stride) {
    if (!e) return FLOWGNN_ERR_ARG;
    // (the shapes are those of the mask, so a mask changed since the run is "not the last run's" too: the caller sized its arrays by it)
    if (!e->ran || !e->attn_mask || e->attn_mask_last != e->attn_mask || (e->G > 0 && (!e->attn_e.last || !e->attn_s.last))) {
        e->err = "flowgnn_get_attention: the last flowgnn_run did not have attention on with this layer mask (flowgnn_set_attention)";
        return FLOWGNN_ERR_STATE;
    }
    int rc = flowgnn_sync(e);
    if (rc) return rc;
    if (e->G == 0) return FLOWGNN_OK;
    const size_t n_sel = (size_t)__builtin_popcount((unsigned)e->attn_mask_last);
    const size_t le = (size_t)e->E * 4, ls = (size_t)e->N * 4;  // floats per layer
    for (size_t k = 0; k < n_sel; k++) {
        if (edge_host && le && (rc = d2h_sync(e, edge_host + k * edge_stride, e->attn_e.last + k * le, sizeof(float) * le, "copy attention (edges)"))) return rc;
        if (self_host && ls && (rc = d2h_sync(e, self_host + k * self_stride, e->attn_s.last + k * ls, sizeof(float) * ls, "copy attention (self)"))) return rc;
    }
    return FLOWGNN_OK;
}

extern "C" {
int flowgnn_get_attention(flowgnn_engine* e, float* edge_host, float* self_host) {
    if (!e) return FLOWGNN_ERR_ARG;
    return get_attention_strided(e, edge_host, (size_t)e->E * 4, self_host, (size_t)e->N * 4);
}

int flowgnn_attention_device(flowgnn_engine* e, void** d_edge, void** d_self) {
    if (!e || (!d_edge && !d_self)) return FLOWGNN_ERR_ARG;
    if (!e->ran || !e->attn_mask || e->attn_mask_last != e->attn_mask || !e->attn_e.last || !e->attn_s.last) {
        e->err = "flowgnn_attention_device: the last flowgnn_run did not have attention on with this layer mask (flowgnn_set_attention)";
        return FLOWGNN_ERR_STATE;
    }
    if (d_edge) *d_edge = e->attn_e.last;
    if (d_self) *d_self = e->attn_s.last;
    return FLOWGNN_OK;
}

int flowgnn_set_attention_buffers(flowgnn_engine* e, void* d_edge, void* d_self) {
    if (int rc = begin_set_buffer(e)) return rc;
    e->attn_e.user = (float*)d_edge;
    e->attn_s.user = (float*)d_self;
    return place_attention(e);
}

int flowgnn_stream(flowgnn_engine* e, void** stream) {
    if (!e || !stream) return FLOWGNN_ERR_ARG;
    *stream = (void*)e->stream;
    return FLOWGNN_OK;
}

int flowgnn_set_stream(flowgnn_engine* e, void* stream, int use_external) {
    if (!e) return FLOWGNN_ERR_ARG;
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();
    EHIP_TRY(e, hipStreamSynchronize(e->stream));
    e->prof.collect();
    e->stream = use_external ? (hipStream_t)stream : e->own_stream;
    return FLOWGNN_OK;
}

int flowgnn_batch_info(const flowgnn_engine* e, long long* num_graphs, long long* total_nodes, long long* total_edges) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (num_graphs) *num_graphs = e->G;
    if (total_nodes) *total_nodes = e->N;
    if (total_edges) *total_edges = e->E;
    return FLOWGNN_OK;
}

int flowgnn_batch_tiles(const flowgnn_engine* e, int* batch_order, int* packed) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (batch_order) *batch_order = e->batch_ready && e->db.gtiles.ok ? e->db.gtiles.n_tiles : 0;
    if (packed) *packed = e->batch_ready && e->db.gtiles.ok ? e->db.gtiles.bp_tiles : 0;
    return FLOWGNN_OK;
}

int flowgnn_exact_reruns(const flowgnn_engine* e) { return e ? e->exact_reruns : -1; }

long long flowgnn_graph_replays(const flowgnn_engine* e) { return e ? e->graph_replays : -1; }

int flowgnn_set_option(flowgnn_engine* e, const char* key, double value) {
    if (!e || !key) return FLOWGNN_ERR_ARG;
    ENGINE_TRY(e, begin_change(e));
    if (!e->opts.set(key, value)) {
        e->err = std::string("flowgnn_set_option: unknown option '") + key + "'";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    e->graph_mode = e->opts.i("hipgraph");
    e->model->configure(e->opts);
    // the batch's graph tiles were packed for the limits the model asked for under the old options: set the batch again
    e->batch_ready = false;
    e->ran = false;
    return FLOWGNN_OK;
}

int flowgnn_get_option(const flowgnn_engine* e, const char* key, double* value) {
    if (!e || !key) return FLOWGNN_ERR_ARG;
    return e->opts.get(key, value) ? FLOWGNN_OK : FLOWGNN_ERR_UNSUPPORTED;
}

int flowgnn_option_count(void) { return kNumOptions; }
const char* flowgnn_option_name(int i) { return (i >= 0 && i < kNumOptions) ? kOptionTable[i].key : nullptr; }

int flowgnn_get_csr(flowgnn_engine* e, int* row_ptr, int* src, int* eid, int* out_deg) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (!e->ran) return FLOWGNN_ERR_STATE;
    ENGINE_TRY(e, use_device(e));
    ensure_csr(e);  // the last run may have worked from the caller's arrays directly
    int rc = flowgnn_sync(e);
    if (rc) return rc;
    if (row_ptr && e->N == 0) row_ptr[0] = 0;  // empty batch: nothing was built (and nothing may have been allocated)
    if (row_ptr && e->N) EHIP_TRY(e, hipMemcpy(row_ptr, e->d_rowptr, sizeof(int) * ((size_t)e->N + 1), hipMemcpyDeviceToHost));
    if (src && e->E) EHIP_TRY(e, hipMemcpy(src, e->d_src, sizeof(int) * (size_t)e->E, hipMemcpyDeviceToHost));
    if (eid && e->E) EHIP_TRY(e, hipMemcpy(eid, e->d_eid, sizeof(int) * (size_t)e->E, hipMemcpyDeviceToHost));
    if (out_deg && e->N) EHIP_TRY(e, hipMemcpy(out_deg, e->d_outdeg, sizeof(int) * (size_t)e->N, hipMemcpyDeviceToHost));
    return FLOWGNN_OK;
}

// The last run kept no per-node rows (a graph-resident kernel, or a readout folded into the last layer): repeat the pass with the
// tap on, on the per-layer kernels -- which also leaves the model's per-batch state of that path (row tiles of the stand-alone
// aggregation kernels) describing THIS batch.  What flowgnn_get_h, flowgnn_get_aggregate and flowgnn_run_aggregation_only read.
static int ensure_rows(flowgnn_engine* e) {
    int rc = flowgnn_sync(e);
    if (rc) return rc;
    if (e->db.h_valid || e->db.tap) return FLOWGNN_OK;
    e->model->set_keep_h(true);
    e->model->set_exact(e->force_exact);
    {   // a tap's pass leaves the run's outputs as they are (of the attention, the models read the mask alone)
        KeepOutputFields keep(e->db);
        for (const Output& o : kOutputs)
            if (o.on) e->db.*o.field = nullptr;
        e->db.attn_mask = 0;
        rc = engine_forward(e);
    }
    e->model->set_keep_h(false);
    if (rc) { e->err = fg::last_error_text(); return rc; }
    return flowgnn_sync(e);
}

int flowgnn_get_h(flowgnn_engine* e, float* h_host, int* dim) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (!e->ran) return FLOWGNN_ERR_STATE;
    int rc = ensure_rows(e);
    if (rc) return rc;
    if (!e->db.h_valid && !e->db.tap) {
        e->err = "flowgnn_get_h: node embeddings are not available as float rows in this numeric mode";
        return FLOWGNN_ERR_UNSUPPORTED;
    }
    const int D = e->db.tap ? e->db.tap_dim : e->model->emb_dim();
    const float* srcp = e->db.tap ? e->db.tap : e->db.h[e->db.final_h];
    if (dim) *dim = D;
    if (h_host && e->N) EHIP_TRY(e, hipMemcpy(h_host, srcp, sizeof(float) * (size_t)e->N * D, hipMemcpyDeviceToHost));
    return FLOWGNN_OK;
}

int flowgnn_profile_enable(flowgnn_engine* e, int on) {
    if (!e) return FLOWGNN_ERR_ARG;
    ENGINE_TRY(e, use_device(e));
    EHIP_TRY(e, hipStreamSynchronize(e->stream));
    e->prof.reset();
    e->prof.enabled = on != 0;
    return FLOWGNN_OK;
}

int flowgnn_profile_read(flowgnn_engine* e, int* count, const char** names, double* total_ms, long long* launches) {
    if (!e || !count) return FLOWGNN_ERR_ARG;
    ENGINE_TRY(e, use_device(e));
    EHIP_TRY(e, hipStreamSynchronize(e->stream));
    e->prof.collect();
    int n = (int)e->prof.names.size();
    if (n > FLOWGNN_MAX_PROFILE_SLOTS) n = FLOWGNN_MAX_PROFILE_SLOTS;
    for (int i = 0; i < n; i++) {
        if (names) names[i] = e->prof.names[i].c_str();
        if (total_ms) total_ms[i] = e->prof.total_ms[i];
        if (launches) launches[i] = e->prof.launches[i];
    }
    *count = n;
    return FLOWGNN_OK;
}

int flowgnn_run_aggregation_only(flowgnn_engine* e, int layer, int iters, float* avg_ms) {
    if (!e || iters <= 0) return FLOWGNN_ERR_ARG;
    if (off_default_width(e)) { e->err = "flowgnn_run_aggregation_only: the engine's width is 300 (flowgnn_set_emb_dim / flowgnn_set_model_emb_dim), which has no stand-alone aggregation kernel"; return FLOWGNN_ERR_UNSUPPORTED; }
    if (!e->ran) { e->err = "flowgnn_run_aggregation_only needs a prior flowgnn_run"; return FLOWGNN_ERR_STATE; }
    if (e->gin_eps_on) { e->err = "flowgnn_run_aggregation_only: a trained eps is on (flowgnn_set_gin_eps), and the stand-alone aggregation kernel has no eps instance"; return FLOWGNN_ERR_UNSUPPORTED; }
    if (e->ogb_vn_on) { e->err = "flowgnn_run_aggregation_only: OGB's virtual node is on (flowgnn_set_ogb_virtual_node / flowgnn_set_gcn_virtual_node), and the stand-alone aggregation kernel does not add it"; return FLOWGNN_ERR_UNSUPPORTED; }
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();
    int rc = e->model->aggregate_dim() > 0 ? ensure_rows(e) : FLOWGNN_OK;  // the kernel's input rows (a resident run left none)
    if (rc) return rc;
    ensure_csr(e);
    rc = e->model->aggregation_only(e->db, layer, e->stream);  // warm-up; also the model's verdict on `layer`
    if (rc) {
        e->err = rc == FLOWGNN_ERR_UNSUPPORTED ? "no standalone aggregation kernel for this model / numeric mode (the fixed-point modes have none)" : "flowgnn_run_aggregation_only: bad layer";
        return rc;
    }
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t he = hipEventCreate(&a);
    if (he == hipSuccess) he = hipEventCreate(&b);
    if (he == hipSuccess) he = hipEventRecord(a, e->stream);
    for (int i = 0; i < iters && he == hipSuccess && rc == 0; i++) rc = e->model->aggregation_only(e->db, layer, e->stream);
    if (he == hipSuccess) he = hipEventRecord(b, e->stream);
    if (he == hipSuccess) he = hipEventSynchronize(b);
    float ms = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (he != hipSuccess) return EHIP_FAIL(e, "flowgnn_run_aggregation_only", he);
    if (rc) { e->err = fg::last_error_text(); return rc; }
    if (avg_ms) *avg_ms = ms / iters;
    return FLOWGNN_OK;
}

int flowgnn_get_aggregate(flowgnn_engine* e, int layer, float* h_in_host, int* in_dim, float* agg_host, int* agg_dim) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (off_default_width(e)) { e->err = "flowgnn_get_aggregate: the engine's width is 300 (flowgnn_set_emb_dim / flowgnn_set_model_emb_dim), which has no stand-alone aggregation kernel"; return FLOWGNN_ERR_UNSUPPORTED; }
    if (!e->ran) { e->err = "flowgnn_get_aggregate needs a prior flowgnn_run"; return FLOWGNN_ERR_STATE; }
    if (e->gin_eps_on) { e->err = "flowgnn_get_aggregate: a trained eps is on (flowgnn_set_gin_eps), and the stand-alone aggregation kernel has no eps instance"; return FLOWGNN_ERR_UNSUPPORTED; }
    if (e->ogb_vn_on) { e->err = "flowgnn_get_aggregate: OGB's virtual node is on (flowgnn_set_ogb_virtual_node / flowgnn_set_gcn_virtual_node), and the stand-alone aggregation kernel does not add it"; return FLOWGNN_ERR_UNSUPPORTED; }
    int rc = flowgnn_sync(e);
    if (rc) return rc;
    e->drop_graph();
    const int D = e->model->emb_dim(), AD = e->model->aggregate_dim();
    if (in_dim) *in_dim = D;
    if (agg_dim) *agg_dim = AD;
    if (AD <= 0) { e->err = "no standalone aggregation kernel for this model / numeric mode (the fixed-point modes have none)"; return FLOWGNN_ERR_UNSUPPORTED; }
    if (e->N == 0 || (!h_in_host && !agg_host)) return FLOWGNN_OK;
    rc = ensure_rows(e);
    if (rc) return rc;
    ensure_csr(e);
    rc = e->model->aggregation_only(e->db, layer, e->stream);
    if (rc) { e->err = rc == FLOWGNN_ERR_UNSUPPORTED ? "flowgnn_get_aggregate: not available in this numeric mode" : "flowgnn_get_aggregate: bad layer"; return rc; }
    EHIP_TRY(e, hipStreamSynchronize(e->stream));
    if (h_in_host)
        EHIP_TRY(e, hipMemcpy(h_in_host, e->db.h[e->db.final_h], sizeof(float) * (size_t)e->N * D, hipMemcpyDeviceToHost));
    if (agg_host) EHIP_TRY(e, hipMemcpy(agg_host, e->db.scratch, sizeof(float) * (size_t)e->N * AD, hipMemcpyDeviceToHost));
    // the model's last launch may have left per-node readout terms in scratch: the next flowgnn_run rewrites them
    return FLOWGNN_OK;
}
}  // extern "C"
