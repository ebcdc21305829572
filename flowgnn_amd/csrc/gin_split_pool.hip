// The graph-resident GIN kernel's pooling instances (flowgnn_set_embeddings): gin_split.hip compiled once more with GS_POOL_TU = 1,
// which leaves gin_resident_pool_kernel<HUBS, F16> -- the un-folded kernel that pools h_5 per graph out of LDS, for both numeric
// modes -- and gin_resident_pool_dispatch.  (GS_SINGLE_PRODUCT = 1 only drops the host-side packers and tile builders, which belong to
// gin_split.hip's own translation unit; the numeric mode of these instances is their template argument.)
#define GS_POOL_TU 1
#define GS_SINGLE_PRODUCT 1
#define gin_resident_kernel gin_resident_pool_kernel
#include "gin_split.hip"
