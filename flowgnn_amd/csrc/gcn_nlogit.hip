// GCN's graph-resident kernel once more, as the instance that also stores every node's term of the readout, a[v] . w + b, in the
// caller's node order (flowgnn_set_node_logits): gcn.hip compiled with FG_RESIDENT_NLOGIT_TU, which leaves launch_gcn_resident_nlogit
// as this translation unit's only symbol.  The kernel carries its own name, so profiles and traces tell the two apart.
#define FG_RESIDENT_NLOGIT_TU 1
#define gcn_resident_kernel gcn_resident_nlogit_kernel
#include "gcn.hip"
