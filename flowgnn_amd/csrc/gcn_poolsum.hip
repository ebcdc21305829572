// GCN's graph-resident kernel once more, as the instance whose readout is the sum of the graph's terms instead of their mean
// (flowgnn_set_pooling, FLOWGNN_POOL_SUM): gcn.hip compiled with FG_RESIDENT_POOLSUM_TU, which leaves launch_gcn_resident_poolsum as this
// translation unit's only symbol.  The kernel carries its own name, so profiles and traces tell the two apart.
#define FG_RESIDENT_POOLSUM_TU 1
#define gcn_resident_kernel gcn_resident_poolsum_kernel
#include "gcn.hip"
