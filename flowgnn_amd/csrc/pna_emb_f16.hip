// The single-product (FLOWGNN_NUMERIC_F16) counterpart of pna_emb.hip: the graph-resident kernel's instance that also stores every
// graph's pooled row, compiled from pna.hip with PNA_SINGLE_PRODUCT = 1.  launch_pna_resident_f16_emb is this translation unit's only symbol.
#define PNA_SINGLE_PRODUCT 1
#define FG_RESIDENT_EMB_TU 1
#define pna_resident_kernel pna_resident_emb_f16_kernel
#include "pna.hip"
