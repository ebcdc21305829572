// The graph-resident GIN kernel's max-pooling instances (flowgnn_set_pooling, FLOWGNN_POOL_MAX): gin_split.hip compiled once more with
// GS_POOL_TU = 1 and GS_POOL_MAX = 1, which leaves gin_resident_poolmax_kernel<HUBS, F16> -- the un-folded pooling kernel whose
// per-(graph, column) chain takes the maximum of the graph's h_5 rows, starting from the graph's first row -- and
// gin_resident_poolmax_dispatch.  It is launched without a logit buffer: the head is applied to the pooled rows by a kernel behind it.
#define GS_POOL_TU 1
#define GS_POOL_MAX 1
#define GS_SINGLE_PRODUCT 1
#define gin_resident_kernel gin_resident_poolmax_kernel
#include "gin_split.hip"
