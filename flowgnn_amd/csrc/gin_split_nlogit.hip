// The graph-resident GIN kernel's node-logit instances (flowgnn_set_node_logits): gin_split.hip compiled once more with GS_NLOGIT_TU = 1,
// which leaves gin_resident_nlogit_kernel<HUBS, ENC, F16> -- the folded kernel that also stores every node's term of the readout, in
// the caller's node order, for both front ends and both numeric modes -- and gin_resident_nlogit_dispatch.  (GS_SINGLE_PRODUCT = 1
// only drops the host-side packers and tile builders, which belong to gin_split.hip's own translation unit; the numeric mode of
// these instances is their template argument.)
#define GS_NLOGIT_TU 1
#define GS_SINGLE_PRODUCT 1
#define gin_resident_kernel gin_resident_nlogit_kernel
#include "gin_split.hip"
