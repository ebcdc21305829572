// GCN's graph-resident kernel once more, as the instance that also stores every node's last-layer row in the caller's node order
// (flowgnn_set_node_embeddings): gcn.hip compiled with FG_RESIDENT_ROWS_TU, which leaves launch_gcn_resident_rows as this
// translation unit's only symbol.  The kernel carries its own name, so profiles and traces tell the two apart.
#define FG_RESIDENT_ROWS_TU 1
#define gcn_resident_kernel gcn_resident_rows_kernel
#include "gcn.hip"
