// The single-product (FLOWGNN_NUMERIC_F16) counterpart of pna_rows.hip: the graph-resident kernel's instance that also stores every
// node's h_4 row, compiled from pna.hip with PNA_SINGLE_PRODUCT = 1.  launch_pna_resident_f16_rows is this translation unit's only symbol.
#define PNA_SINGLE_PRODUCT 1
#define FG_RESIDENT_ROWS_TU 1
#define pna_resident_kernel pna_resident_rows_f16_kernel
#include "pna.hip"
