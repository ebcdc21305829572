// Single-product instances of DGN's matrix-pipe kernels (FLOWGNN_NUMERIC_F16): dgn.hip compiled once more with
// DGN_SINGLE_PRODUCT = 1.  Every operand of a matrix-pipe product -- the transposed source rows, the directional weights, the eight
// a1 / a2 values a lane feeds into a K-step, the scaled update weights -- is one f16 value (round to nearest even), and every product is
// one f16 MFMA (fp32 accumulate); see dgn.hip (DGN_OPER2, put_row_piece, the K-step) for what changes.  The kernels carry their own
// names, so profiles and traces tell the two modes apart.  This translation unit holds the graph-resident default instance and the
// per-layer matrix-pipe kernel's three instances, behind launch_dgn_*_f16.
#define DGN_SINGLE_PRODUCT 1
#define dgn_resident_kernel dgn_resident_f16_kernel
#define dgn_layer_mfma_kernel dgn_layer_mfma_f16_kernel
#include "dgn.hip"
