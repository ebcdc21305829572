// wide_vocab_score.h -- code2's vocabulary head scoring given target tokens (flowgnn_set_vocab_targets): the
// launchers of wide_vocab_score.hip's kernels.  GwReadout (wide_common.h) calls them only while the head is on and targets are
// attached to the batch: in every other state no launch comes from here.  emb_dim: 300, the one instantiation (anything else:
// FLOWGNN_ERR_UNSUPPORTED).  `blob` is the head's own device form (wide_vocab.h), `plan` is vocab_head_plan's.
#pragma once
#include "common.h"
#include "wide_vocab.h"

namespace fg {

// What a run with targets t [G][P] (int32, -1: no target at this position) leaves beside tokens / scores, all [G][P]:
//   logit: the head's logit at t (NaN where t is -1), with the bits the stream pass computes for that entry
//   lse:   log sum_v exp(logit[v]), section 4.34's
//   rank:  how many entries v != t come before t under (larger value, then lower index); -1 where t is -1
struct VocabScore {
    const int* targets;
    float* logit;
    float* lse;
    int* rank;
};

// part, in 4-byte words: the targets' logits in the scaled domain [G][P] (what the stream pass compares against), then, with more than
// one slice, (value, index, count, m, s) per [slice][graph][position]: section 4.33's pairs and three words more
size_t vocab_score_part_words(const VocabHeadPlan& plan, int num_graphs, int positions);

// The gathered-row product: logit and part's first [G][P] from the target rows of the head's chunks.  A target outside -1 .. V - 1
// raises *err (ERR_NODE_FEAT) and counts as -1; a pooled value out of range raises *range_flag, as launch_vocab_head does
int launch_vocab_target(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, void* part,
                        const VocabScore& sc, int* err, int* range_flag, hipStream_t s);
// The stream pass: launch_vocab_head's tokens and scores, bit for bit, and beside them lse and rank; with plan.slices > 1 the slices'
// partial results go to `part` and launch_vocab_score_fold follows
int launch_vocab_score(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                       void* part, int* tokens, float* scores, const VocabScore& sc, int* range_flag, hipStream_t s);
int launch_vocab_score_fold(int emb_dim, const void* blob, int positions, int vocab, const VocabHeadPlan& plan, const void* part, int num_graphs,
                            int* tokens, float* scores, const VocabScore& sc, hipStream_t s);
// The exact form (the repeated pass behind the range guard): launch_vocab_head_f32's fma chain for everything, the target's logit included
int launch_vocab_score_f32(int emb_dim, const void* blob, int positions, int vocab, const float* pooled, int num_graphs, int* tokens, float* scores,
                           const VocabScore& sc, int* err, hipStream_t s);

}  // namespace fg
