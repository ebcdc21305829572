// GAT's graph-resident kernel once more, as the instance that also stores the attention coefficients of the selected layers
// (flowgnn_set_attention): gat.hip compiled with FG_RESIDENT_ATTN_TU, which leaves launch_gat_resident_attn as this translation unit's
// only symbol.  The kernel carries its own name, so profiles and traces tell the instances apart; it stores the node logits too when
// they are on, so the two features together keep the one launch.
#define FG_RESIDENT_ATTN_TU 1
#define gat_resident_kernel gat_resident_attn_kernel
#include "gat.hip"
