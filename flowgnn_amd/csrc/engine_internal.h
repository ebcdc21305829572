// engine_internal.h -- what engine.hip, engine_config.hip, group.hip and entry.hip share beyond the C ABI of include/flowgnn.h: the
// engine and group objects, the buffer helper and the slot type of the optional outputs, the macros that carry a failure's text to the
// engine, the list of the optional outputs (kOutputs), and the few functions of engine.hip that the other files call (for
// engine_config.hip: use_device, begin_change).
#pragma once
#include "common.h"
#include "../../include/flowgnn.h"
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace fg {
void set_last_error(const char* what);
int option_index(const char* key);  // index into the option table of engine.hip, -1: no such option
// THE place where the library reads its environment (engine.hip)
void read_environment(std::vector<double>* option_values, std::vector<int>* devices, bool* stale_num_task = nullptr);

// A device buffer (pinned: a pinned host buffer) that only grows.
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    bool pinned = false;
    bool holds(size_t bytes) const { return p && bytes <= cap; }
    // at least `bytes` (never null afterwards); headroom: a regrow takes an eighth more than asked for, for callers whose sizes differ by
    // a few percent from call to call (the ranges of a cut job)
    hipError_t reserve(size_t bytes, bool headroom) {
        if (holds(bytes)) return hipSuccess;
        release();
        const size_t want = (bytes ? bytes : 1) + (headroom ? bytes / 8 : 0);
        const hipError_t he = pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (he == hipSuccess) cap = want; else p = nullptr;
        return he;
    }
    void release() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
};

// The engine-side state of ONE optional per-run output (graph embeddings, node embeddings, node logits, GAT's attention
// coefficients of the edges and of the self edges); its switch is the engine's (*_on, attn_mask).  The rules, for all of them:
// off by default, and the DeviceBatch pointer it feeds is null then, so every forward is the one it was; `own` is allocated when
// first needed, to one batch's size, and outlives the batch; `user` is the caller's buffer (flowgnn_set_*_buffer), which
// flowgnn_set_batch forgets; `last` is where the last flowgnn_run put the result (null: it ran with the output off) -- what a get
// copies and the *_device calls return.  engine.hip: `place`; the list kOutputs is below.
struct OutSlot {
    GrowBuf own;
    float* user = nullptr;
    float* last = nullptr;
    float* target(bool on) const { return on ? (user ? user : (float*)own.p) : nullptr; }
};
}  // namespace fg

struct flowgnn_engine {
    int model_id = 0;
    int device = 0;
    hipStream_t stream = nullptr;      // the stream every launch goes to
    hipStream_t own_stream = nullptr;  // the engine's own stream (stream == own_stream unless flowgnn_set_stream redirected it)
    hipStream_t copy_stream = nullptr; // flowgnn_set_batch's host -> device copies: the engine's own queue, not the process's null stream
    fg::Model* model = nullptr;
    fg::Options opts;   // defaults <- environment (read once, here) <- flowgnn_set_option
    fg::Profiler prof;
    std::string err;

    // resident batch
    bool batch_ready = false;
    bool ran = false;
    int num_tasks = 1;          // NUM_TASK of the readout: results are [G][num_tasks]
    int emb_dim = 0;            // the width of the engine's embeddings: flowgnn_embedding_dim(model) at flowgnn_create, then what flowgnn_set_emb_dim (GIN) / flowgnn_set_model_emb_dim (GIN, GCN) said
    bool force_exact = false;   // the resident batch tripped the range flag once: run it on the exact kernels
    int exact_reruns = 0;
    long long G = 0, N = 0, E = 0;
    double job_fill = -1.0;            // flowgnn_set_job_tile_fill: the graph-tile fill of the JOB (-1: the batch's own packing decides)
    long long job_n = -1, job_e = -1;  // flowgnn_set_job_totals: the job the next batches are shards of (-1: each batch is its own job)
    int max_nodes = 0, max_edges = 0;
    size_t capG = 0, capN = 0, capE = 0;
    int *d_nn = nullptr, *d_ne = nullptr, *d_noff = nullptr, *d_eoff = nullptr;
    int *d_nf = nullptr, *d_el = nullptr, *d_ea = nullptr;
    float* d_eig = nullptr;
    int *d_rowptr = nullptr, *d_src = nullptr, *d_eid = nullptr, *d_outdeg = nullptr, *d_gsrc = nullptr, *d_gdst = nullptr,
        *d_cursor = nullptr, *d_tmp = nullptr, *d_bsums = nullptr, *d_err = nullptr;
    uint8_t* d_ecode = nullptr;
    float *d_h0 = nullptr, *d_h1 = nullptr, *d_scratch = nullptr, *d_out = nullptr;
    fg::GrowBuf tiles;  // GraphTiles::row_start | graph_start in one allocation
    fg::GrowBuf bp;     // GraphTiles::bp_list | bp_lrow | bp_graph | bp_row in one allocation
    fg::GrowBuf sub;    // GraphTiles::sub | big_row | big_graph in one allocation
    fg::GrowBuf h_pack{nullptr, 0, true}, d_pack;  // packed host -> device transfer (h2d_pack.cpp): pinned staging + its device copy
    bool has_attr = false, has_eig = false;
    fg::DeviceBatch db{};

    // flowgnn_laplacian_eigen*: no part of the resident batch.  eig_plan: node / edge offsets and the three size-class lists of the
    // call, in one allocation; eig_io: the host function's edge list and output on the device; eig_done: behind the last call's
    // kernels on the launch stream (the next call waits for it before it rewrites eig_plan)
    fg::GrowBuf eig_plan, eig_io;
    hipEvent_t eig_done = nullptr;

    int numeric_mode = FLOWGNN_NUMERIC_F32;
    int pooling = FLOWGNN_POOL_MEAN;  // flowgnn_set_pooling: the engine's, across batches (db.pooling follows it)
    bool gin_eps_on = false;          // flowgnn_set_gin_eps: the engine's too, across batches and weight sets (db.gin_eps_on / gin_self_scale follow)
    float gin_eps[FLOWGNN_MAX_NUM_LAYERS] = {};
    bool ogb_vn_on = false;           // flowgnn_set_ogb_virtual_node: the engine's as well (db.ogb_vn follows it)
    fg::GrowBuf ogb_vn;               // ... and its five tensors on the device (gin_ogbvn.h: GIN_OGBVN_FLOATS)
    bool attn_pool_on = false;        // flowgnn_set_attention_pooling: the engine's as well (db.attn_pool follows it)
    fg::GrowBuf attn_pool;            // ... and the gate's three tensors on the device (wide_attn.h)
    int s2s_steps = 0;                // flowgnn_set_set2set_pooling: the engine's as well, 0 = off (db.s2s / db.s2s_steps follow it)
    fg::GrowBuf s2s;                  // ... and its six tensors on the device (wide_s2s.h)
    int jk = FLOWGNN_JK_LAST;         // flowgnn_set_jk_residual: the engine's as well, across batches and weight sets (db.jk / db.residual follow)
    int residual = 0;
    int num_layers = FLOWGNN_NUM_LAYERS_DEFAULT;  // flowgnn_set_num_layers: the model's depth (GIN, GCN at width 300: 2 .. 8); sizes eps and the virtual node's tensors
    static_assert(FLOWGNN_MAX_NUM_LAYERS == fg::MAX_NUM_LAYERS && FLOWGNN_NUM_LAYERS_DEFAULT == fg::NUM_LAYERS_DEFAULT, "common.h restates the header's two depths");

    // the optional outputs (fg::OutSlot): graph embeddings [G][dim] (flowgnn_set_embeddings), node embeddings [N][dim]
    // (flowgnn_set_node_embeddings), node logits [N][num_tasks] (flowgnn_set_node_logits) and, for GAT, the attention coefficients
    // [n_sel][E][4] and [n_sel][N][4], n_sel = popcount(attn_mask) (flowgnn_set_attention): the mask is the switch of both, and the
    // mask of the last run is kept beside where it put them (the shapes a get copies are that run's)
    bool emb_on = false, nemb_on = false, nlog_on = false;
    int attn_mask = 0, attn_mask_last = 0;
    fg::OutSlot emb, nemb, nlog, attn_e, attn_s;

    // hipGraph replay of the launch sequence (index build + forward), opt-in (FLOWGNN_HIPGRAPH=1; 2 = batches of any size).
    // Measured on this runtime it does not pay: asynchronous launches already pipeline, and a replay of the dozen kernels
    // of a step is 1-4 % SLOWER than launching them (4 113 molhiv graphs: 0.267 ms plain, 0.271 ms replayed; 512 graphs:
    // 0.099 vs 0.103 ms) -- so it is off by default and kept for hosts whose launch path is the bottleneck.
    // The first run of a batch is plain (models size their scratch buffers there), the second is captured, later ones
    // replay.  Every call that changes what the captured kernels would read or write drops the recording.
    hipGraphExec_t gexec = nullptr;
    bool graph_ok = false;
    bool graph_h_valid = true;   // what the captured forward left in db.h_valid / tap / tap_dim / final_h (host-side outputs)
    const float* graph_tap = nullptr;
    int graph_tap_dim = 0, graph_final_h = 0;
    int plain_runs = 0;
    int graph_mode = 0;  // option hipgraph
    long long graph_replays = 0;
    void drop_graph() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        gexec = nullptr;
        graph_ok = false;
        plain_runs = 0;
    }

    void free_batch() {
        void* ptrs[] = {d_nn /* base of d_ne, d_noff, d_eoff too */, d_nf, d_el, d_ea, d_eig, d_rowptr, d_src, d_eid, d_outdeg, d_gsrc,
                        d_gdst, d_cursor, d_tmp, d_bsums, d_ecode, d_h0, d_h1, d_scratch, d_out};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        d_nn = d_ne = d_noff = d_eoff = d_nf = d_el = d_ea = nullptr;
        d_eig = nullptr;
        d_rowptr = d_src = d_eid = d_outdeg = d_gsrc = d_gdst = d_cursor = d_tmp = d_bsums = nullptr;
        d_ecode = nullptr;
        d_h0 = d_h1 = d_scratch = d_out = nullptr;
        for (fg::GrowBuf* b : {&tiles, &bp, &sub, &h_pack, &d_pack}) b->release();
        capG = capN = capE = 0;
    }
};

// ---- engine.hip, for engine_config.hip
int use_device(flowgnn_engine* e);
// what every call that changes what the launched kernels read starts with: the engine's device, no recorded launch sequence, an idle stream
int begin_change(flowgnn_engine* e);
// the engine is GIN or GCN at width 300 (flowgnn_emb_dim is the model's own figure otherwise: 100, GAT's 16, PNA's 80)
inline bool off_default_width(const flowgnn_engine* e) { return e->emb_dim != flowgnn_embedding_dim(e->model_id); }

// The optional per-run outputs (fg::OutSlot above), in ONE list: everything that treats them alike walks it.  (static: a list with
// external linkage would be compiled for the device as well, where the functions it points to do not exist.)
struct Output {
    fg::OutSlot flowgnn_engine::*slot;
    float* fg::DeviceBatch::*field;           // the pointer of the forward's DeviceBatch that the slot feeds
    bool flowgnn_engine::*on;                 // its switch (null: attn_mask, the switch of both attention slots)
    size_t (*floats)(const flowgnn_engine*);  // what the resident batch needs of it
    const char *noun, *setter;                // for the texts of its get and *_device calls
    const char* no_fixed_point;               // flowgnn_set_numeric_mode's refusal while it is on (null: the row above has said it)
};
inline size_t emb_dim_of(const flowgnn_engine* e) { return (size_t)e->emb_dim; }  // the ENGINE's width (flowgnn_set_emb_dim), not the model's default
inline size_t attn_layers(const flowgnn_engine* e) { return (size_t)__builtin_popcount((unsigned)e->attn_mask); }
enum { OUT_EMB, OUT_NEMB, OUT_NLOG, OUT_ATTN_E, OUT_ATTN_S };
static const Output kOutputs[] = {
    {&flowgnn_engine::emb, &fg::DeviceBatch::emb, &flowgnn_engine::emb_on, [](const flowgnn_engine* e) { return (size_t)e->G * emb_dim_of(e); },
     "embeddings", "flowgnn_set_embeddings", "flowgnn_set_numeric_mode: graph embeddings are on, and there are no fixed-point embeddings"},
    {&flowgnn_engine::nemb, &fg::DeviceBatch::node_emb, &flowgnn_engine::nemb_on, [](const flowgnn_engine* e) { return (size_t)e->N * emb_dim_of(e); },
     "node embeddings", "flowgnn_set_node_embeddings", "flowgnn_set_numeric_mode: node embeddings are on, and there are no fixed-point node embeddings"},
    {&flowgnn_engine::nlog, &fg::DeviceBatch::node_logits, &flowgnn_engine::nlog_on, [](const flowgnn_engine* e) { return (size_t)e->N * (size_t)e->num_tasks; },
     "node logits", "flowgnn_set_node_logits", "flowgnn_set_numeric_mode: node logits are on, and there are no fixed-point node logits"},
    {&flowgnn_engine::attn_e, &fg::DeviceBatch::attn_edge, nullptr, [](const flowgnn_engine* e) { return attn_layers(e) * (size_t)e->E * 4; },
     "attention", "flowgnn_set_attention", "flowgnn_set_numeric_mode: attention is on, and there are no fixed-point attention coefficients"},
    {&flowgnn_engine::attn_s, &fg::DeviceBatch::attn_self, nullptr, [](const flowgnn_engine* e) { return attn_layers(e) * (size_t)e->N * 4; },
     "attention", "flowgnn_set_attention", nullptr},
};
inline bool is_on(const flowgnn_engine* e, const Output& o) { return o.on ? e->*o.on : e->attn_mask != 0; }

#define ENGINE_TRY(e, expr)                                     \
    do {                                                        \
        int _rc = (expr);                                       \
        if (_rc) { (e)->err = fg::last_error_text(); return _rc; } \
    } while (0)

// HIP call made in an engine context: the failure text goes to the thread-local slot AND to the engine, so
// flowgnn_last_error(e) always reports the latest failure (never a stale earlier one)
#define EHIP_TRY(e, expr)                                                   \
    do {                                                                    \
        hipError_t _he = (expr);                                            \
        if (_he != hipSuccess) {                                            \
            fg::set_hip_error(#expr, _he, __FILE__, __LINE__);              \
            (e)->err = fg::last_error_text();                               \
            return FLOWGNN_ERR_HIP;                                         \
        }                                                                   \
    } while (0)

// ... and a failed HIP call the caller has a text of its own for: the status to return
#define EHIP_FAIL(e, what, he) (fg::set_hip_error(what, he, __FILE__, __LINE__), (e)->err = fg::last_error_text(), (int)FLOWGNN_ERR_HIP)

// fill of the model's graph tiles when the graphs are packed greedily in batch order (flowgnn_graph_tile_fill)
double graph_tile_fill(fg::Model* model, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges);
// flowgnn_set_batch with copy_mu (flowgnn_group_compute): held around the large host -> device copies only -- one copier per DEVICE at
// a time, while another engine of the same device packs its next range on the host or plans its tiles
int set_batch_impl(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, const int* node_feature,
                   const int* edge_list, const int* edge_attr, const float* node_eigen, std::mutex* copy_mu);

// flowgnn_get_attention with the distance, in floats, between two selected layers of each host array (the group's members write their
// edge / node range of every layer into the job's arrays)
int get_attention_strided(flowgnn_engine* e, float* edge_host, size_t edge_stride, float* self_host, size_t self_stride);

class GroupWorkers;  // group.hip
struct flowgnn_group {
    ~flowgnn_group();
    int model_id = 0;
    std::unique_ptr<GroupWorkers> workers;
    std::mutex call_mu;  // one group call at a time (the workers hold one function)
    std::vector<flowgnn_engine*> eng;
    std::vector<int> cut;  // [n + 1] graph cuts of the resident batch
    bool batch_valid = false;  // the engines hold the shards `cut` describes (flowgnn_group_set_batch); flowgnn_group_compute and the
                               // entry points leave each engine on its LAST range and clear this
    std::vector<std::unique_ptr<std::mutex>> copy_mu;  // flowgnn_group_compute: one copier per device ...
    std::vector<int> copy_of;                          // ... engine i uses copy_mu[copy_of[i]] (the first engine on its device)
    int num_tasks = 1;
    std::string err;
};
