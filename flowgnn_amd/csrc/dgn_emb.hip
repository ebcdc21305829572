// DGN's graph-resident kernel once more, as the instance that also stores every graph's pooled row (flowgnn_set_embeddings):
// dgn.hip compiled with FG_RESIDENT_EMB_TU, which leaves launch_dgn_resident_emb as this translation unit's only symbol.  The kernel
// carries its own name, so profiles and traces tell the two apart.
#define FG_RESIDENT_EMB_TU 1
#define dgn_resident_kernel dgn_resident_emb_kernel
#include "dgn.hip"
