// Single-product instances of PNA's split kernels (FLOWGNN_NUMERIC_F16): pna.hip compiled once more with
// PNA_SINGLE_PRODUCT = 1.  Each of the eight values a lane feeds into a K-step is one f16 value (round to nearest even), the weights are
// the hi halves alone, and every product is one f16 MFMA (fp32 accumulate); see pna.hip (PNA_OPER2, pna_stream_mfma) for what changes.
// The kernels carry their own names, so profiles and traces tell the two modes apart.  This translation unit holds the graph-resident
// default instance, the per-layer fused kernel and the two-kernel layer's dense kernel, behind launch_pna_*_f16.
#define PNA_SINGLE_PRODUCT 1
#define pna_resident_kernel pna_resident_f16_kernel
#define pna_layer_fused_kernel pna_layer_fused_f16_kernel
#define pna_dense_split_kernel pna_dense_split_f16_kernel
#include "pna.hip"
