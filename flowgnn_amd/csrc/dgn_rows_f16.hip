// The single-product (FLOWGNN_NUMERIC_F16) counterpart of dgn_rows.hip: the graph-resident kernel's instance that also stores every
// node's h_4 row, compiled from dgn.hip with DGN_SINGLE_PRODUCT = 1.  launch_dgn_resident_f16_rows is this translation unit's only symbol.
#define DGN_SINGLE_PRODUCT 1
#define FG_RESIDENT_ROWS_TU 1
#define dgn_resident_kernel dgn_resident_rows_f16_kernel
#include "dgn.hip"
