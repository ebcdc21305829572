// Single-product instances of GIN's split kernels (FLOWGNN_NUMERIC_F16): gin_split.hip compiled once more with GS_SINGLE_PRODUCT = 1.
// Every MLP operand is one f16 value (round to nearest even) and every product one f16 MFMA (fp32 accumulate); see gin_split.hip
// (GS_OPER2) for what changes.  The kernels carry their own names, so profiles and traces tell the two modes apart.
#define GS_SINGLE_PRODUCT 1
#define gin_layer_split_kernel gin_layer_split_f16_kernel
#define gin_resident_kernel gin_resident_f16_kernel
#include "gin_split.hip"
