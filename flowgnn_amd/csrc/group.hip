// group.hip -- several devices behind one handle: flowgnn_group_*, flowgnn_shard_ranges, flowgnn_create_multi.
// north_star: "that batch dimension is partitioned across the 8 GPUs of one node".  A group = one engine (own stream, own
// resident shard) per listed device + one host thread per engine for every call that touches the device; the batch is cut
// into contiguous graph ranges balanced by sum(N + E) (flowgnn_shard_ranges, the C counterpart of flowgnn_amd/dist.py) and
// the results are written into the caller's buffer in job order.  A device may be listed more than once (two engines on
// one GPU: what the 1-GPU tests do) -- graphs are independent, so results are bit-identical to the single-engine run.
#include "engine_internal.h"
#include <atomic>
#include <condition_variable>
#include <thread>

// One persistent host thread per engine (engine 0 runs on the caller's thread): a call that touches the devices hands every worker the
// same function and waits for all of them.  (Creating and joining a std::thread per engine and call -- what this replaced -- costs
// 60-100 us per call with eight engines; a dataset-sized step is 190 us of GPU time.)  Workers spin briefly for the next job before
// they sleep on the condition variable, so the timed loop of `host --devices` (flowgnn_group_run back to back) never pays a wake-up.
class GroupWorkers {
public:
    ~GroupWorkers() { stop(); }
    void start(int n_engines) {
        n_ = n_engines;
        rc_.assign((size_t)n_engines, 0);
        for (int i = 1; i < n_engines; i++) th_.emplace_back([this, i] { loop(i); });
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_go_.notify_all();
        for (auto& t : th_) t.join();
        th_.clear();
    }
    // fn(i) for every engine i; returns the per-engine status codes
    const std::vector<int>& each(const std::function<int(int)>& fn) {
        if (n_ > 1) {
            {
                std::lock_guard<std::mutex> lk(mu_);
                fn_ = &fn;
                pending_.store(n_ - 1, std::memory_order_relaxed);
                gen_.fetch_add(1, std::memory_order_release);
            }
            cv_go_.notify_all();
        }
        // engine 0 runs here, on the caller's thread: its hipSetDevice must not outlive the call (the caller's current device is the
        // caller's business), and whatever fn(0) throws (std::bad_alloc from a staging vector) the workers still hold &fn and write
        // rc_ -- so the wait below runs before anything leaves this frame, and the exception becomes a status code (this is a C ABI)
        int caller_dev = -1;
        const bool have_dev = hipGetDevice(&caller_dev) == hipSuccess;
        try {
            rc_[0] = fn(0);
        } catch (...) {
            rc_[0] = FLOWGNN_ERR_HIP;
        }
        if (n_ > 1) {
            for (int spin = 0; spin < 20000 && pending_.load(std::memory_order_acquire) > 0; spin++) cpu_relax();
            if (pending_.load(std::memory_order_acquire) > 0) {
                std::unique_lock<std::mutex> lk(mu_);
                cv_done_.wait(lk, [this] { return pending_.load(std::memory_order_acquire) == 0; });
            }
            fn_ = nullptr;
        }
        if (have_dev) (void)hipSetDevice(caller_dev);
        return rc_;
    }

private:
    static void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
    }
    void loop(int i) {
        unsigned long long seen = 0;
        while (true) {
            // a short spin (a back-to-back caller is here again within microseconds), then sleep
            for (int spin = 0; spin < 4000 && gen_.load(std::memory_order_acquire) == seen; spin++) cpu_relax();
            if (gen_.load(std::memory_order_acquire) == seen) {
                std::unique_lock<std::mutex> lk(mu_);
                cv_go_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen; });
            }
            const std::function<int(int)>* fn;
            {
                std::lock_guard<std::mutex> lk(mu_);  // pairs with each(): fn_ and gen_ are published together
                seen = gen_.load(std::memory_order_acquire);
                if (quit_) return;
                fn = fn_;
            }
            try {
                rc_[(size_t)i] = (*fn)(i);
            } catch (...) {
                rc_[(size_t)i] = FLOWGNN_ERR_HIP;  // (an exception must not end the worker with the caller still waiting for it)
            }
            if (pending_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                std::lock_guard<std::mutex> lk(mu_);
                cv_done_.notify_one();
            }
        }
    }
    int n_ = 0;
    std::vector<std::thread> th_;
    std::vector<int> rc_;
    std::mutex mu_;
    std::condition_variable cv_go_, cv_done_;
    const std::function<int(int)>* fn_ = nullptr;
    std::atomic<unsigned long long> gen_{0};
    std::atomic<int> pending_{0};
    bool quit_ = false;
};

flowgnn_group::~flowgnn_group() = default;

namespace {
int group_each(flowgnn_group* g, const std::function<int(int)>& fn) {  // fn(i) on every engine, each on its own (persistent) host thread; first failure wins
    const int n = (int)g->eng.size();
    std::lock_guard<std::mutex> call(g->call_mu);
    const std::vector<int>& rc = g->workers->each(fn);
    for (int i = 0; i < n; i++)
        if (rc[(size_t)i]) {
            g->err = "engine " + std::to_string(i) + " (device " + std::to_string(g->eng[(size_t)i]->device) + "): " + flowgnn_last_error(g->eng[(size_t)i]);
            return rc[(size_t)i];
        }
    return FLOWGNN_OK;
}
// a call that is the same engine call on every member
int group_all(flowgnn_group* g, const std::function<int(flowgnn_engine*)>& fn) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    return group_each(g, [&](int i) { return fn(g->eng[(size_t)i]); });
}
// every flowgnn_group_* call starts with no error text of an earlier call; argument errors leave their own
int group_fail(flowgnn_group* g, int rc, const char* what) {
    if (g) g->err = what;
    fg::set_last_error(what);
    return rc;
}
// node / edge offsets at every cut (the reference's running nodes_offset / edges_offset, GIN/src/GIN_compute.cc:96-97)
void offsets_at_cuts(const std::vector<int>& cut, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                     std::vector<long long>* noff, std::vector<long long>* eoff) {
    noff->assign(cut.size(), 0);
    eoff->assign(cut.size(), 0);
    long long N = 0, E = 0;
    size_t r = 0;
    for (int gi = 0; gi <= num_graphs; gi++) {
        while (r < cut.size() && cut[r] == gi) { (*noff)[r] = N; (*eoff)[r] = E; r++; }
        if (gi < num_graphs) { N += nums_of_nodes[gi]; E += nums_of_edges[gi]; }
    }
}
// A member's batches are shards of the group's JOB while this lives: every shard chooses its kernels by the job's totals and tile fill,
// the same kernels as one engine holding all of it.  Afterwards a flowgnn_set_batch on the member itself is its own job again.
struct JobScope {
    flowgnn_engine* const e;
    const long long keep_n = e->job_n, keep_e = e->job_e;
    const double keep_fill = e->job_fill;
    JobScope(flowgnn_engine* e_, long long job_n, long long job_e, double job_fill) : e(e_) {
        flowgnn_set_job_totals(e, job_n, job_e);
        flowgnn_set_job_tile_fill(e, job_fill);
    }
    ~JobScope() { e->job_n = keep_n; e->job_e = keep_e; e->job_fill = keep_fill; }
};
}  // namespace

extern "C" {

int flowgnn_shard_ranges(int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, int parts, int* cuts) {
    if (num_graphs < 0 || parts < 1 || !cuts || (num_graphs > 0 && (!nums_of_nodes || !nums_of_edges))) return FLOWGNN_ERR_ARG;
    long long total = 0;
    for (int g = 0; g < num_graphs; g++) total += (long long)nums_of_nodes[g] + nums_of_edges[g];
    // cut r = the first graph index whose cumulative work reaches r / parts of the total (exact integer comparison)
    cuts[0] = 0;
    long long cum = 0;
    int g = 0;
    for (int r = 1; r < parts; r++) {
        while (g < num_graphs && cum * parts < total * r) { cum += (long long)nums_of_nodes[g] + nums_of_edges[g]; g++; }
        cuts[r] = g;
    }
    cuts[parts] = num_graphs;
    return FLOWGNN_OK;
}

int flowgnn_create_multi(int model, int n_devices, const int* device_ids, flowgnn_group** out) {
    if (!out || n_devices < 1 || !device_ids) return FLOWGNN_ERR_ARG;
    *out = nullptr;
    flowgnn_group* g = new flowgnn_group();
    g->model_id = model;
    for (int i = 0; i < n_devices; i++) {
        flowgnn_engine* e = nullptr;
        const int rc = flowgnn_create(model, device_ids[i], &e);
        if (rc) {
            for (auto* p : g->eng) flowgnn_destroy(p);
            delete g;
            return rc;
        }
        g->eng.push_back(e);
    }
    g->cut.assign((size_t)n_devices + 1, 0);
    g->workers.reset(new GroupWorkers());
    g->workers->start(n_devices);
    for (int i = 0; i < n_devices; i++) {
        int first = i;
        for (int k = 0; k < i; k++)
            if (device_ids[k] == device_ids[i]) { first = k; break; }
        g->copy_of.push_back(first);
        g->copy_mu.emplace_back(new std::mutex());
    }
    *out = g;
    return FLOWGNN_OK;
}

int flowgnn_group_destroy(flowgnn_group* g) {
    if (!g) return FLOWGNN_ERR_ARG;
    if (g->workers) g->workers->stop();
    for (auto* e : g->eng) flowgnn_destroy(e);
    delete g;
    return FLOWGNN_OK;
}

int flowgnn_group_size(const flowgnn_group* g) { return g ? (int)g->eng.size() : -1; }
flowgnn_engine* flowgnn_group_engine(flowgnn_group* g, int i) { return (g && i >= 0 && i < (int)g->eng.size()) ? g->eng[(size_t)i] : nullptr; }
const char* flowgnn_group_last_error(const flowgnn_group* g) { return (g && !g->err.empty()) ? g->err.c_str() : fg::last_error_text(); }

int flowgnn_group_set_weights(flowgnn_group* g, int count, const float* const* tensors) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_weights(e, count, tensors); }); }
int flowgnn_group_load_weights_dir(flowgnn_group* g, const char* dir) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_load_weights_dir(e, dir); }); }
int flowgnn_group_set_option(flowgnn_group* g, const char* key, double value) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_option(e, key, value); }); }
int flowgnn_group_set_num_tasks(flowgnn_group* g, int num_tasks) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    const int rc = group_each(g, [&](int i) { return flowgnn_set_num_tasks(g->eng[(size_t)i], num_tasks); });
    if (!rc) g->num_tasks = num_tasks;
    return rc;
}
int flowgnn_group_set_emb_dim(flowgnn_group* g, int emb_dim) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    for (flowgnn_engine* e : g->eng)
        if (e->emb_dim != emb_dim) g->batch_valid = false;  // (a member that changes its width drops its shard with it)
    return group_each(g, [&](int i) { return flowgnn_set_emb_dim(g->eng[(size_t)i], emb_dim); });
}
int flowgnn_group_set_model_emb_dim(flowgnn_group* g, int emb_dim) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    for (flowgnn_engine* e : g->eng)
        if (e->emb_dim != emb_dim) g->batch_valid = false;  // (as above)
    return group_each(g, [&](int i) { return flowgnn_set_model_emb_dim(g->eng[(size_t)i], emb_dim); });
}
int flowgnn_group_set_numeric_mode(flowgnn_group* g, int mode) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_numeric_mode(e, mode); }); }
int flowgnn_group_set_numeric_mode_dim(flowgnn_group* g, int emb_dim, int mode) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_numeric_mode_dim(e, emb_dim, mode); });
}
int flowgnn_group_set_model_numeric_mode_dim(flowgnn_group* g, int emb_dim, int mode) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_model_numeric_mode_dim(e, emb_dim, mode); });
}
int flowgnn_group_set_model_numeric_mode(flowgnn_group* g, int model_id, int mode) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_model_numeric_mode(e, model_id, mode); });
}
int flowgnn_group_set_pooling(flowgnn_group* g, int mode) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_pooling(e, mode); }); }
int flowgnn_group_set_gin_eps(flowgnn_group* g, const float* eps) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_gin_eps(e, eps); }); }
int flowgnn_group_set_ogb_virtual_node(flowgnn_group* g, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_ogb_virtual_node(e, vn_embedding, w1, b1, w2, b2); });
}

int flowgnn_group_set_ogb_virtual_node_dim(flowgnn_group* g, int emb_dim, const float* vn_embedding, const float* w1, const float* b1, const float* w2,
                                           const float* b2) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_ogb_virtual_node_dim(e, emb_dim, vn_embedding, w1, b1, w2, b2); });
}

int flowgnn_group_set_gcn_virtual_node(flowgnn_group* g, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_gcn_virtual_node(e, vn_embedding, w1, b1, w2, b2); });
}

int flowgnn_group_set_gcn_virtual_node_dim(flowgnn_group* g, int emb_dim, const float* vn_embedding, const float* w1, const float* b1, const float* w2,
                                           const float* b2) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_gcn_virtual_node_dim(e, emb_dim, vn_embedding, w1, b1, w2, b2); });
}

int flowgnn_group_set_attention_pooling(flowgnn_group* g, int emb_dim, const float* w1, const float* b1, const float* w2) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_attention_pooling(e, emb_dim, w1, b1, w2); });
}

int flowgnn_group_set_set2set_pooling(flowgnn_group* g, int emb_dim, int steps, int num_tasks, const float* w_ih, const float* w_hh,
                                      const float* b_ih, const float* b_hh, const float* head_w, const float* head_b) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_set2set_pooling(e, emb_dim, steps, num_tasks, w_ih, w_hh, b_ih, b_hh, head_w, head_b); });
}

int flowgnn_group_set_jk_residual(flowgnn_group* g, int emb_dim, int jk, int residual) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_jk_residual(e, emb_dim, jk, residual); });
}

int flowgnn_group_set_model_jk_residual(flowgnn_group* g, int emb_dim, int jk, int residual) {
    return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_model_jk_residual(e, emb_dim, jk, residual); });
}

// (a member that changes its depth drops its shard with it, as with the width)
int flowgnn_group_set_num_layers(flowgnn_group* g, int emb_dim, int num_layers) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    for (flowgnn_engine* e : g->eng)
        if (e->num_layers != num_layers) g->batch_valid = false;
    return group_each(g, [&](int i) { return flowgnn_set_num_layers(g->eng[(size_t)i], emb_dim, num_layers); });
}

int flowgnn_group_set_embeddings(flowgnn_group* g, int on) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_embeddings(e, on); }); }
int flowgnn_group_set_node_embeddings(flowgnn_group* g, int on) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_node_embeddings(e, on); }); }
int flowgnn_group_set_node_logits(flowgnn_group* g, int on) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_node_logits(e, on); }); }

int flowgnn_group_set_attention(flowgnn_group* g, int layer_mask) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_set_attention(e, layer_mask); }); }

int flowgnn_group_set_batch(flowgnn_group* g, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                            const int* node_feature, const int* edge_list, const int* edge_attr, const float* node_eigen) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    g->batch_valid = false;
    if (num_graphs < 0) return group_fail(g, FLOWGNN_ERR_ARG, "flowgnn_group_set_batch: negative graph count");
    if (num_graphs > 0 && (!nums_of_nodes || !nums_of_edges)) return group_fail(g, FLOWGNN_ERR_ARG, "flowgnn_group_set_batch: null count arrays");
    const int n = (int)g->eng.size();
    g->cut.assign((size_t)n + 1, 0);
    int rc = flowgnn_shard_ranges(num_graphs, nums_of_nodes, nums_of_edges, n, g->cut.data());
    if (rc) return group_fail(g, rc, "flowgnn_group_set_batch: flowgnn_shard_ranges refused the counts");
    std::vector<long long> noff, eoff;
    offsets_at_cuts(g->cut, num_graphs, nums_of_nodes, nums_of_edges, &noff, &eoff);
    const double job_fill = graph_tile_fill(g->eng[0]->model, num_graphs, nums_of_nodes, nums_of_edges);  // (the members are one model with one option set)
    rc = group_each(g, [&](int i) {
        const int g0 = g->cut[(size_t)i], g1 = g->cut[(size_t)i + 1];
        const long long n0 = noff[(size_t)i], e0 = eoff[(size_t)i];
        flowgnn_engine* e = g->eng[(size_t)i];
        JobScope job(e, noff[(size_t)n], eoff[(size_t)n], job_fill);
        return flowgnn_set_batch(e, g1 - g0, nums_of_nodes ? nums_of_nodes + g0 : nullptr,
                                 nums_of_edges ? nums_of_edges + g0 : nullptr, node_feature ? node_feature + n0 * 9 : nullptr,
                                 edge_list ? edge_list + e0 * 2 : nullptr, edge_attr ? edge_attr + e0 * 3 : nullptr,
                                 node_eigen ? node_eigen + n0 * 4 : nullptr);
    });
    g->batch_valid = rc == FLOWGNN_OK;
    return rc;
}

// the members still hold the shards flowgnn_group_set_batch gave them?  (flowgnn_group_engine hands the members out for per-engine
// calls: a flowgnn_set_batch on one of them would otherwise have its rows copied to the old cut's offset)
static int group_shards_intact(flowgnn_group* g, const char* who) {
    for (size_t i = 0; i < g->eng.size(); i++)
        if (g->eng[i]->G != g->cut[i + 1] - g->cut[i]) {
            g->batch_valid = false;
            const std::string msg = std::string(who) + ": engine " + std::to_string(i) + " no longer holds its shard of the group's batch (a per-engine flowgnn_set_batch?); call flowgnn_group_set_batch again";
            return group_fail(g, FLOWGNN_ERR_STATE, msg.c_str());
        }
    return FLOWGNN_OK;
}

int flowgnn_group_shards(const flowgnn_group* g, int* cuts) {
    if (!g || !cuts) return FLOWGNN_ERR_ARG;
    if (!g->batch_valid) { fg::set_last_error("flowgnn_group_shards: no batch set by flowgnn_group_set_batch"); return FLOWGNN_ERR_STATE; }
    for (size_t i = 0; i < g->cut.size(); i++) cuts[i] = g->cut[i];
    return FLOWGNN_OK;
}

int flowgnn_group_run(flowgnn_group* g) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    if (!g->batch_valid) return group_fail(g, FLOWGNN_ERR_STATE, "flowgnn_group_run: no batch set by flowgnn_group_set_batch (flowgnn_group_compute and the entry points leave none)");
    if (int rc = group_shards_intact(g, "flowgnn_group_run")) return rc;
    return group_each(g, [&](int i) { return flowgnn_run(g->eng[(size_t)i]); });
}
int flowgnn_group_sync(flowgnn_group* g) { return group_all(g, [&](flowgnn_engine* e) { return flowgnn_sync(e); }); }
int flowgnn_group_get_results(flowgnn_group* g, float* out_host) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    if (!g->batch_valid) return group_fail(g, FLOWGNN_ERR_STATE, "flowgnn_group_get_results: no batch set by flowgnn_group_set_batch (flowgnn_group_compute and the entry points leave none)");
    if (int rc = group_shards_intact(g, "flowgnn_group_get_results")) return rc;
    if (!out_host && g->cut.back() > 0) return group_fail(g, FLOWGNN_ERR_ARG, "flowgnn_group_get_results: null output");
    return group_each(g, [&](int i) {
        flowgnn_engine* e = g->eng[(size_t)i];
        if (e->G == 0) return flowgnn_sync(e);
        return flowgnn_get_results(e, out_host + (size_t)g->cut[(size_t)i] * g->num_tasks);
    });
}

// first[i]: where member i's rows (graphs: &flowgnn_engine::G, nodes: N, edges: E) start in the job, first.back(): the job's
// (the shards are contiguous graph ranges, so member i's rows start where the rows of members 0 .. i - 1 end)
static std::vector<size_t> first_rows(const flowgnn_group* g, long long flowgnn_engine::*rows) {
    std::vector<size_t> first(1, 0);
    if (g)
        for (const flowgnn_engine* e : g->eng) first.push_back(first.back() + (size_t)(e->*rows));
    return first;
}

// What the group's gets of the optional outputs share: the shards must be those of flowgnn_group_set_batch, `have_out` false is
// an error when the job has rows (first.back(), as first_rows counts them), and a member with an empty shard only synchronises --
// if `on` says it has the output on.  get(e, i): the member's own get, into its place of the job's array.
static int group_get_output(flowgnn_group* g, const char* who, bool have_out, const std::vector<size_t>& first,
                            const std::function<bool(const flowgnn_engine*)>& on, const std::function<int(flowgnn_engine*, size_t)>& get) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    if (!g->batch_valid) return group_fail(g, FLOWGNN_ERR_STATE, (std::string(who) + ": no batch set by flowgnn_group_set_batch (flowgnn_group_compute and the entry points leave none)").c_str());
    if (int rc = group_shards_intact(g, who)) return rc;
    if (!have_out && first.back() > 0) return group_fail(g, FLOWGNN_ERR_ARG, (std::string(who) + ": null output").c_str());
    return group_each(g, [&](int i) {
        flowgnn_engine* e = g->eng[(size_t)i];
        if (e->G == 0) return on(e) ? flowgnn_sync(e) : (int)FLOWGNN_ERR_STATE;
        return get(e, (size_t)i);
    });
}

int flowgnn_group_get_embeddings(flowgnn_group* g, float* out_host) {
    const std::vector<size_t> first = first_rows(g, &flowgnn_engine::G);
    return group_get_output(g, "flowgnn_group_get_embeddings", out_host != nullptr, first, [](const flowgnn_engine* e) { return e->emb_on; },
                            [&](flowgnn_engine* e, size_t i) { return flowgnn_get_embeddings(e, out_host + first[i] * (size_t)flowgnn_emb_dim(e)); });
}

// [N_tot][dim] in job order
int flowgnn_group_get_node_embeddings(flowgnn_group* g, float* out_host) {
    const std::vector<size_t> first = first_rows(g, &flowgnn_engine::N);
    return group_get_output(g, "flowgnn_group_get_node_embeddings", out_host != nullptr, first, [](const flowgnn_engine* e) { return e->nemb_on; },
                            [&](flowgnn_engine* e, size_t i) { return flowgnn_get_node_embeddings(e, out_host + first[i] * (size_t)flowgnn_emb_dim(e)); });
}

// [N_tot][NUM_TASK] in job order, likewise
int flowgnn_group_get_node_logits(flowgnn_group* g, float* out_host) {
    const std::vector<size_t> first = first_rows(g, &flowgnn_engine::N);
    return group_get_output(g, "flowgnn_group_get_node_logits", out_host != nullptr, first, [](const flowgnn_engine* e) { return e->nlog_on; },
                            [&](flowgnn_engine* e, size_t i) { return flowgnn_get_node_logits(e, out_host + first[i] * (size_t)e->num_tasks); });
}

// [n_sel][E_tot][4] and [n_sel][N_tot][4] in job order: per selected layer, member i's edges / nodes start where those of members
// 0 .. i - 1 end (edge indices are the caller's, per graph range); either array may be null
int flowgnn_group_get_attention(flowgnn_group* g, float* edge_host, float* self_host) {
    const std::vector<size_t> nfirst = first_rows(g, &flowgnn_engine::N), efirst = first_rows(g, &flowgnn_engine::E);
    return group_get_output(g, "flowgnn_group_get_attention", true, nfirst, [](const flowgnn_engine* e) { return e->attn_mask != 0; },
                            [&](flowgnn_engine* e, size_t i) {
                                return get_attention_strided(e, edge_host ? edge_host + efirst[i] * 4 : nullptr, efirst.back() * 4,
                                                             self_host ? self_host + nfirst[i] * 4 : nullptr, nfirst.back() * 4);
                            });
}

// One call for a batch that lives in HOST memory: the job is cut into size x chunks_per_engine ranges (same rule), and engine i
// takes ranges i, i + size, ... one after the other -- set_batch (validation, tile packing, host -> device), run, results into
// out_host at the range's place.  While one engine's kernels run, the other engines' copies are in flight: with two engines on ONE
// device the PCIe transfer of range j + 1 hides under the kernels of range j (the entry points do exactly that).  The engines are
// left holding their last range.
int flowgnn_group_compute(flowgnn_group* g, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                          const int* node_feature, const int* edge_list, const int* edge_attr, const float* node_eigen,
                          float* out_host, int chunks_per_engine) {
    if (!g) return FLOWGNN_ERR_ARG;
    g->err.clear();
    if (num_graphs < 0 || chunks_per_engine < 1) return group_fail(g, FLOWGNN_ERR_ARG, "flowgnn_group_compute: negative graph count or chunks_per_engine < 1");
    if (num_graphs > 0 && (!nums_of_nodes || !nums_of_edges || !out_host)) return group_fail(g, FLOWGNN_ERR_ARG, "flowgnn_group_compute: null count arrays or output");
    const int n = (int)g->eng.size();
    const int S = n * chunks_per_engine;
    std::vector<int> cut((size_t)S + 1, 0);
    int rc = flowgnn_shard_ranges(num_graphs, nums_of_nodes, nums_of_edges, S, cut.data());
    if (rc) return group_fail(g, rc, "flowgnn_group_compute: flowgnn_shard_ranges refused the counts");
    // the engines end up holding their LAST range, not the shards of a flowgnn_group_set_batch job: run / get_results / shards
    // answer FLOWGNN_ERR_STATE until the next flowgnn_group_set_batch
    g->batch_valid = false;
    g->cut.assign((size_t)n + 1, 0);
    std::vector<long long> noff, eoff;
    offsets_at_cuts(cut, num_graphs, nums_of_nodes, nums_of_edges, &noff, &eoff);
    const int T = g->num_tasks;
    const double job_fill = graph_tile_fill(g->eng[0]->model, num_graphs, nums_of_nodes, nums_of_edges);  // (the members are one model with one option set)
    return group_each(g, [&](int i) {
        flowgnn_engine* e = g->eng[(size_t)i];
        JobScope job(e, noff[(size_t)S], eoff[(size_t)S], job_fill);
        for (int j = i; j < S; j += n) {
            const int g0 = cut[(size_t)j], g1 = cut[(size_t)j + 1];
            if (g1 == g0) continue;
            const long long n0 = noff[(size_t)j], e0 = eoff[(size_t)j];
            int r;
            // one host -> device copy per DEVICE at a time (the mutex is taken inside, around the copies only: the host-side packing of
            // this range runs under the other engine's copy): two threads copying from pageable memory to the same GPU get a quarter
            // of the rate each (6.0 ms against 1.4 for a 67 MB range), and the ranges would then march in lockstep instead of
            // alternating copy / kernels
            r = set_batch_impl(e, g1 - g0, nums_of_nodes + g0, nums_of_edges + g0, node_feature ? node_feature + n0 * 9 : nullptr,
                               edge_list ? edge_list + e0 * 2 : nullptr, edge_attr ? edge_attr + e0 * 3 : nullptr,
                               node_eigen ? node_eigen + n0 * 4 : nullptr, g->copy_mu[(size_t)g->copy_of[(size_t)i]].get());
            if (!r) r = flowgnn_run(e);
            if (!r) r = flowgnn_get_results(e, out_host + (size_t)g0 * T);
            if (r) return r;
        }
        return (int)FLOWGNN_OK;
    });
}

}  // extern "C"
