// gin_resident_launch.h -- what launch_gin_resident (gin_split.h) is asked for and which of the resident kernel's compiled instances that
// selects: plain C++ (no HIP, no engine), so a CPU test can pin the selection.
#pragma once
#include <cstdint>

namespace fg {

struct GinTileBuild;  // gin_split.h

// The arguments of launch_gin_resident.  h0 = atom-encoder output [N][100]; row_ptr / src / ecode = the CSR (all four null with tb: the
// tile loader reads the caller's arrays); out [G] receives the logits.
struct GinResidentLaunch {
    const float* h0 = nullptr;
    float* hout = nullptr;  // h_5 rows for the flowgnn_get_h tap (un-folds the readout)
    const int* row_ptr = nullptr;
    const int* src = nullptr;
    const uint8_t* ecode = nullptr;
    const float* ecomb_all = nullptr;     // [5][60][100]
    const uint8_t* chunks_all = nullptr;  // 5 x gin_resident_layer_bytes()
    const float* pool_w = nullptr;
    const float* pool_b = nullptr;
    const int* tile_row = nullptr;
    const int* tile_graph = nullptr;
    uint8_t* tile_desc = nullptr;  // scratch, n_tiles x GIN_RESIDENT_DESC_BYTES
    const int* node_off = nullptr;
    float* out = nullptr;
    int n_tiles = 0;
    int* range_flag = nullptr;
    bool hubs = false;
    const float* head_u = nullptr;  // gin_resident_head_fold's output: with out and no hout, the folded single-task readout
    int col_order = 0;
    bool prof = false;                 // development aid: the phase breakdown of the default instance, printed per launch (synchronises!)
    const GinTileBuild* tb = nullptr;  // the one-pass front end (folded forms only)
    int tstride = 1;                   // 2: tile_row / tile_graph are (start, end) pair lists
    bool f16 = false;                  // single-product instances, FLOWGNN_NUMERIC_F16
    float* emb = nullptr;          // [G][100]: the per-graph mean of the h_5 rows, pooled inside the un-folded kernel (out [G] required)
    float* node_logits = nullptr;  // [N]: every node's term of the folded readout, caller order (folded forms only: head_u, out, no hout)
    // FLOWGNN_POOL_*.  1 (sum): the folded forms' instances whose readout leaves the division out -- the caller passes it only with head_u,
    // out and no hout / emb / node_logits.  2 (max): with emb, the pooling instance that leaves the per-column maxima of h_5 there and
    // writes no logit -- the caller applies the head to emb
    int pooling = 0;
    // flowgnn_set_gin_eps: s_l = 1 + eps[l] of the five layers (host).  The eps instances (gin_resident_eps_kernel): folded forms only,
    // pooling 0, no hout / emb / node_logits
    const float* self_scale = nullptr;
};

// the translation unit whose kernels run: gin_split.hip / gin_split_f16.hip, then gin_split_<name>.hip
enum class GinResidentInstance { Default, Eps, PoolMean, PoolMax, PoolSum, NodeLogits, Refused };

struct GinResidentPick {
    GinResidentInstance instance;
    bool fold;  // single-task readout folded into the last layer, no per-node tap
    bool enc;   // descriptor + encoder indices straight from the caller's arrays, h_0 computed by the tile loader (fold only)
    const char* refusal;  // Refused: fg::last_error_text's message, else null
};

inline GinResidentPick gin_resident_pick(const GinResidentLaunch& a) {
    const bool pool = a.emb != nullptr;  // the pooling instances: un-folded, no tap, no phase stamps -- head_u and hout are not looked at
    const bool fold = !pool && a.head_u != nullptr && a.out != nullptr && a.hout == nullptr;
    const bool enc = a.tb != nullptr && fold;
    const bool extra = pool || a.node_logits != nullptr;
    // a mode other than the mean has the instances named below and no other: anything else would be the mean's logits under its name
    if (a.pooling != 0 && !(a.pooling == 1 && fold && !extra) && !(a.pooling == 2 && pool))
        return {GinResidentInstance::Refused, fold, enc,
                "launch_gin_resident: pooling 1 (sum) runs the folded instances only (head_u, out, no hout / emb / node_logits), pooling 2 (max) "
                "the pooling instance only (emb)"};
    // eps on: the folded, single-task, mean-pooling instances and no other -- anything else would be the eps-less model under its name
    if (a.self_scale != nullptr && !(fold && a.pooling == 0 && !extra && a.tstride == 1))
        return {GinResidentInstance::Refused, fold, enc,
                "launch_gin_resident: a trained eps runs the folded mean-pooling instances only (head_u, out, no hout / emb / node_logits)"};
    GinResidentInstance i = GinResidentInstance::Default;
    if (a.self_scale != nullptr) i = GinResidentInstance::Eps;
    else if (pool) i = a.pooling == 2 ? GinResidentInstance::PoolMax : GinResidentInstance::PoolMean;
    else if (a.pooling == 1) i = GinResidentInstance::PoolSum;  // (past the refusals: folded, no node_logits)
    else if (a.node_logits != nullptr && fold) i = GinResidentInstance::NodeLogits;
    return {i, fold, enc, nullptr};
}

}  // namespace fg
