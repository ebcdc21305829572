// wide_vocab.h -- ogbg-code2 on the 300-wide GIN: the vocabulary head with its fused argmax
// (flowgnn_set_vocab_head) and the AST node encoder (flowgnn_set_ast_encoder).  The device forms of their tensors and the launchers of
// wide_vocab.hip's kernels.  GwReadout (wide_common.h) calls the head's launcher only while the head is on and GinWideModel
// (gin_wide.hip) the encoder's only while the encoder is on: in the default state no launch comes from here.  emb_dim: 300, the one
// instantiation (anything else: 0 bytes / FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"

namespace fg {

// The head: logit[g][p][v] = b[p][v] + W[p][v] . pooled[g], token[g][p] = argmax_v (the lowest v among equal logits), score[g][p] the
// maximum.  The device form of w [P][V][D] and b [P][V], in bytes (every part a multiple of 16), VT = ceil(V / 16):
//   P x VT chunks of VH_CHUNK_STRIDE bytes: the A operands of tile (p, t), 10 K-steps x {hi, lo} x 1 KiB in gw_pack_tile's layout,
//       times one power-of-two scale, then the tile's 16 biases times that scale
//   | 1 / scale, padded to 16 bytes | W^T [P][D][V4] | b [P][V4]     (V4 = V rounded up to 4; the two fp32 parts: the exact form)
size_t vocab_head_blob_bytes(int emb_dim, int positions, int vocab);
void vocab_head_blob_pack(int emb_dim, int positions, int vocab, const float* w, const float* b, void* out);

// How the launch is cut for G graphs on a device of `cus` compute units: blocks of 128 graphs and vocabulary slices (section 4.33).
// part: (float, int) per [slice][graph][position], what the launch below needs while slices > 1 (vocab_head_part_words: its size in
// 4-byte words, 0 for one slice)
struct VocabHeadPlan {
    int slices, graph_blocks;
};
VocabHeadPlan vocab_head_plan(int num_graphs, int vocab, int cus);
// k: flowgnn_set_vocab_topk's (0: the argmax form).  The top-k form's part: K (float, int) pairs and one (m, s) pair per
// [slice][graph][position]
size_t vocab_head_part_words(const VocabHeadPlan& plan, int num_graphs, int positions, int k = 0);

// pooled [G][D] -> tokens [G][P], scores [G][P].  exact: the fp32 VALU form (a plain fma chain, k ascending).  Otherwise the split-f16
// matrix-pipe kernel, which raises *range_flag when a pooled value is at or beyond 6e4 or not finite; with plan.slices > 1 launch_vocab_head_fold
// follows and folds the slices' partial maxima (two calls: each launch has a profile slot of its own in the caller)
int launch_vocab_head(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                      void* part, int* tokens, float* scores, int* range_flag, hipStream_t s);
int launch_vocab_head_fold(int emb_dim, const void* blob, int positions, int vocab, const VocabHeadPlan& plan, const void* part, int num_graphs,
                           int* tokens, float* scores, hipStream_t s);
int launch_vocab_head_f32(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, int* tokens, float* scores,
                          hipStream_t s);

// The top-k form of the three (flowgnn_set_vocab_topk): beside tokens / scores (rank 0, the bits of the
// launchers above) the k best entries of every position under the same order -- larger value, then lower index; token -1 and score
// -inf at ranks beyond the vocabulary -- and lse = log sum_v exp(logit).  The same plan, the same range rule, a part sized with k
struct VocabTopk {
    int k;          // 1 .. FLOWGNN_MAX_VOCAB_TOPK
    int* tokens;    // [G][P][k]
    float* scores;  // [G][P][k]
    float* lse;     // [G][P]
};
int launch_vocab_topk(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                      void* part, int* tokens, float* scores, const VocabTopk& top, int* range_flag, hipStream_t s);
int launch_vocab_topk_fold(int emb_dim, const void* blob, int positions, int vocab, const VocabHeadPlan& plan, const void* part, int num_graphs,
                           int* tokens, float* scores, const VocabTopk& top, hipStream_t s);
int launch_vocab_topk_f32(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, int* tokens, float* scores,
                          const VocabTopk& top, hipStream_t s);

// The AST node encoder: h0[v] = type_tab[x[v][0]] + attr_tab[x[v][1]] + depth_tab[min(depth[v], max_depth)] (+ vn_e, the virtual
// node's E, when non-null), in that order.  The device form: type_tab [n_types][D] | attr_tab [n_attrs][D] | depth_tab [max_depth + 1][D]
size_t ast_encoder_blob_bytes(int emb_dim, int n_types, int n_attrs, int max_depth);
void ast_encoder_blob_pack(int emb_dim, int n_types, int n_attrs, int max_depth, const float* type_tab, const float* attr_tab, const float* depth_tab,
                           void* out);
int launch_ast_encoder(int emb_dim, const void* blob, int n_types, int n_attrs, int max_depth, const int* x, const int* depth, float* h, int n_tot,
                       int* err, const float* vn_e, hipStream_t s);

}  // namespace fg
