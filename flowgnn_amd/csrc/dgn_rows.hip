// DGN's graph-resident kernel once more, as the instance that also stores every node's h_4 row in the caller's node order
// (flowgnn_set_node_embeddings): dgn.hip compiled with FG_RESIDENT_ROWS_TU, which leaves launch_dgn_resident_rows as this
// translation unit's only symbol.  The kernel carries its own name, so profiles and traces tell the two apart.
#define FG_RESIDENT_ROWS_TU 1
#define dgn_resident_kernel dgn_resident_rows_kernel
#include "dgn.hip"
