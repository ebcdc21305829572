// GAT's graph-resident kernel once more, as the instance whose readout is the sum of the graph's terms instead of their mean
// (flowgnn_set_pooling, FLOWGNN_POOL_SUM): gat.hip compiled with FG_RESIDENT_POOLSUM_TU, which leaves launch_gat_resident_poolsum as this
// translation unit's only symbol.  The kernel carries its own name, so profiles and traces tell the two apart.
#define FG_RESIDENT_POOLSUM_TU 1
#define gat_resident_kernel gat_resident_poolsum_kernel
#include "gat.hip"
