// The graph-resident GIN kernel's sum-pooling instances (flowgnn_set_pooling, FLOWGNN_POOL_SUM): gin_split.hip compiled once more with
// GS_POOLSUM_TU = 1, which leaves gin_resident_poolsum_kernel<HUBS, ENC, F16> -- the folded kernel whose readout is the sum of the
// graph's terms plus n_g times the folded head's constant, for both front ends and both numeric modes -- and
// gin_resident_poolsum_dispatch.  (GS_SINGLE_PRODUCT = 1 only drops the host-side packers and tile builders, which belong to
// gin_split.hip's own translation unit; the numeric mode of these instances is their template argument.)
#define GS_POOLSUM_TU 1
#define GS_SINGLE_PRODUCT 1
#define gin_resident_kernel gin_resident_poolsum_kernel
#include "gin_split.hip"
