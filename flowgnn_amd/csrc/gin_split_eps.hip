// The graph-resident GIN kernel's eps instances (flowgnn_set_gin_eps): gin_split.hip compiled once more with GS_EPS_TU = 1, which leaves
// gin_resident_eps_kernel<HUBS, ENC, F16> -- the folded, single-task, mean-pooling kernel whose self term is s_l h[v], s_l = 1 + eps[l]
// by value in the argument block, for both front ends and both numeric modes --, gin_layer_split_eps_kernel<NT, WAVES, F16> -- the
// per-layer kernel with s_l as one more argument, for every configuration the resident instances do not cover -- and their two
// launchers, gin_resident_eps_dispatch and launch_gin_layer_split_eps.  (GS_SINGLE_PRODUCT = 1
// only drops the host-side packers and tile builders, which belong to gin_split.hip's own translation unit; the numeric mode of these
// instances is their template argument.)
#define GS_EPS_TU 1
#define GS_SINGLE_PRODUCT 1
#define gin_resident_kernel gin_resident_eps_kernel
#define gin_layer_split_kernel gin_layer_split_eps_kernel
#include "gin_split.hip"
