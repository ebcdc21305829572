// wide_vocab_f16.h -- code2's vocabulary head in its f16 numeric mode (flowgnn_set_vocab_head_numeric): the
// device form of its weight stream and the launcher of wide_vocab_f16.hip's kernel.  GwReadout (wide_common.h) calls the launcher only
// while the head is on in that mode: in the default state no launch comes from here.  emb_dim: 300, the one instantiation (anything
// else: 0 bytes / FLOWGNN_ERR_UNSUPPORTED).
#pragma once
#include "common.h"
#include "wide_vocab.h"

namespace fg {

// The head's f16 rule: logit[g][p][v] = (b[p][v] s + sum_k r(W[p][v][k] s) r(pooled[g][k])) / s, s the head's power-of-two scale, r to
// nearest even to f16, the sum fp32 on the matrix pipe from the pre-scaled bias: ONE product per K-step where wide_vocab.hip has three.
// The stream, in bytes, VC = ceil(ceil(V / 16) / 2) chunks per position:
//   P x VC chunks of VHF_CHUNK_STRIDE bytes: two 16-row vocabulary tiles each, a tile as its 10 hi fragments of 1 KiB in
//       gw_pack_tile's layout and then its 16 pre-scaled biases; the second tile of a position's last chunk is zero when VT is odd
//   | 1 / scale, padded to 16 bytes
// It is cut out of the head's own device form (`blob`: a host copy of vocab_head_blob_pack's output, its chunk part and 1 / scale are
// what is read), so the hi halves are gw_put_split's, bit for bit.
size_t vocab_head_f16_blob_bytes(int emb_dim, int positions, int vocab);
// ... and how much of `blob`, from its start, vocab_head_f16_blob_pack reads
size_t vocab_head_f16_source_bytes(int emb_dim, int positions, int vocab);
void vocab_head_f16_blob_pack(int emb_dim, int positions, int vocab, const void* blob, void* out);

// How this form's launch is cut: blocks of 128 T graphs (T: the graph tiles a wave holds, a constant of the kernel) and vocabulary
// slices of a whole number of chunks -- an even number of tiles, at least four, none empty.  The part and its fold are section 4.33's:
// vocab_head_part_words and launch_vocab_head_fold take this plan as they take vocab_head_plan's.
VocabHeadPlan vocab_head_f16_plan(int num_graphs, int vocab, int cus);
int vocab_head_f16_graph_tiles();  // T

// pooled [G][D] -> tokens [G][P], scores [G][P] (one slice) or the slices' partial pairs in `part`, which launch_vocab_head_fold then
// folds.  Raises *range_flag under section 4.33's rule; the engine then repeats the pass and the head runs launch_vocab_head_f32
int launch_vocab_head_f16(int emb_dim, const void* stream, int positions, int vocab, const float* pooled, int num_graphs, const VocabHeadPlan& plan,
                          void* part, int* tokens, float* scores, int* range_flag, hipStream_t s);

}  // namespace fg
