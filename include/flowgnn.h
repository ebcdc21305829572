/*
 * flowgnn.h -- C ABI of the MI355X-native FlowGNN inference engine.
 *
 * This is the drop-in boundary for FlowGNN's NT/MP hot path.  Two layers:
 *
 *  (1) Reference-compatible entry points  <M>_compute_graphs(...)
 *      Same symbol names and argument order as the reference's HLS kernels
 *      (cited per function; paths relative to the reference repo), with `float` in
 *      place of FM_TYPE/WT_TYPE (ap_fixed<16,6>) and `int` status instead of `void`.
 *      All pointers are caller-owned HOST buffers; `out` is written on return.
 *      Graphs are concatenated with node ids LOCAL to each graph, exactly as the
 *      reference host builds them (GIN/src/host.cc:119-138).
 *
 *  (2) Handle API  flowgnn_*  (what (1) is implemented on)
 *      One engine per GPU, one HIP stream per engine; weights and the graph batch
 *      stay resident in HBM across runs, so a caller can time the device path
 *      alone, as the reference times kernel execution alone (run_experiments.sh:44).
 *
 * No torch / C++ types cross this boundary: plain pointers and sizes only.
 */
#ifndef FLOWGNN_H
#define FLOWGNN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference returns void and never checks) ---- */
#define FLOWGNN_OK 0
#define FLOWGNN_ERR_ARG 1          /* null pointer, negative count, num_nodes <= 0 */
#define FLOWGNN_ERR_EDGE_RANGE 2   /* edge endpoint outside [0, num_nodes) of its graph */
#define FLOWGNN_ERR_EDGE_ATTR 3    /* edge attribute outside its embedding table */
#define FLOWGNN_ERR_NODE_FEAT 4    /* node feature outside its embedding table */
#define FLOWGNN_ERR_HIP 5          /* HIP runtime error (see flowgnn_last_error) */
#define FLOWGNN_ERR_STATE 6        /* weights or batch not set */
#define FLOWGNN_ERR_IO 7           /* weight / graph file missing or short */
#define FLOWGNN_ERR_UNSUPPORTED 8  /* also: a graph larger than 2 048 nodes / 16 384 edges with a node of more than 16 384 in-edges */

/* ---- model ids ---- */
#define FLOWGNN_MODEL_GIN 0
#define FLOWGNN_MODEL_GIN_VN 1 /* same kernel as GIN; host appends a virtual node (GIN-VN/src/host_load.cc:125-153) */
#define FLOWGNN_MODEL_GCN 2
#define FLOWGNN_MODEL_GAT 3
#define FLOWGNN_MODEL_PNA 4
#define FLOWGNN_MODEL_DGN 5

/* ---- fixed model constants (GIN/src/dcl.h:16-26) ---- */
#define FLOWGNN_ND_FEATURE 9
#define FLOWGNN_ND_FEATURE_TOTAL 173
#define FLOWGNN_EDGE_ATTR 3
#define FLOWGNN_ED_FEATURE_PER_LAYER 13

/* =====================================================================
 * (1) Reference-compatible entry points
 * ===================================================================== */

/*
 * Replaces GIN_compute_graphs, GIN/src/dcl.h:75-94 (def. GIN/src/GIN_compute.cc:7-99);
 * also the GIN-VN kernel (GIN-VN/src/dcl.h, byte-identical).
 *   out                      [num_graphs][1]
 *   node_feature_in          int [N_tot][9]
 *   edge_list_in             int [E_tot][2]  (u, v): h[u] is sent to v
 *   edge_attr_in             int [E_tot][3]
 *   *_weight*                leading dimension = weight-set index, selected by the
 *                            running count of reload_weights[] (GIN_compute.cc:51-53)
 *   node_embedding_weight_in [S][173][100]   edge_embedding_weight_in [S][5][13][100]
 *   node_mlp_1_weights [S][5][200][100]  node_mlp_1_bias [S][5][200]
 *   node_mlp_2_weights [S][5][100][200]  node_mlp_2_bias [S][5][100]
 *   graph_pred_weights_in [S][1][100]    graph_pred_bias_in [S][1]
 */
int GIN_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges,
                       int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in, int* edge_attr_in,
                       float* node_embedding_weight_in, float* edge_embedding_weight_in,
                       float* node_mlp_1_weights, float* node_mlp_1_bias,
                       float* node_mlp_2_weights, float* node_mlp_2_bias,
                       float* graph_pred_weights_in, float* graph_pred_bias_in);

/*
 * NUM_TASK (a compile-time constant of the reference build, GIN/src/dcl.h:25, 1 as shipped; ogbg-molpcba has 128) as an explicit
 * last argument: graph_pred_weights_in is then [S][num_tasks][100], graph_pred_bias_in [S][num_tasks], out [num_graphs][num_tasks]
 * (`FM_TYPE out[][NUM_TASK]`, GIN/src/dcl.h:80).  GIN_compute_graphs(...) == GIN_compute_graphs_mt(..., 1); nothing about the
 * shape of `out` is ever taken from the environment.
 */
int GIN_compute_graphs_mt(int num_graphs, int* nums_of_nodes, int* nums_of_edges,
                          int* reload_weights, float* out,
                          int* node_feature_in, int* edge_list_in, int* edge_attr_in,
                          float* node_embedding_weight_in, float* edge_embedding_weight_in,
                          float* node_mlp_1_weights, float* node_mlp_1_bias,
                          float* node_mlp_2_weights, float* node_mlp_2_bias,
                          float* graph_pred_weights_in, float* graph_pred_bias_in, int num_tasks);

/*
 * Replaces GCN_compute_graphs, GCN/src/dcl.h:75-97 (def. GCN/src/GCN_compute.cc:7-112).
 *   out [num_graphs]; graph arrays as for GIN
 *   convs_weight_in [S][5][100][100]  convs_bias_in [S][5][100]  convs_root_emb_weight_in [S][5][100]
 *   bn_weight_in / bn_bias_in / bn_mean_in / bn_var_in [S][5][100]   (eval-mode BatchNorm)
 */
int GCN_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges,
                       int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in, int* edge_attr_in,
                       float* node_embedding_weight_in, float* edge_embedding_weight_in,
                       float* convs_weight_in, float* convs_bias_in, float* convs_root_emb_weight_in,
                       float* bn_weight_in, float* bn_bias_in, float* bn_mean_in, float* bn_var_in,
                       float* graph_pred_weights_in, float* graph_pred_bias_in);

/* GCN with NUM_TASK as an explicit last argument (see GIN_compute_graphs_mt). */
int GCN_compute_graphs_mt(int num_graphs, int* nums_of_nodes, int* nums_of_edges,
                          int* reload_weights, float* out,
                          int* node_feature_in, int* edge_list_in, int* edge_attr_in,
                          float* node_embedding_weight_in, float* edge_embedding_weight_in,
                          float* convs_weight_in, float* convs_bias_in, float* convs_root_emb_weight_in,
                          float* bn_weight_in, float* bn_bias_in, float* bn_mean_in, float* bn_var_in,
                          float* graph_pred_weights_in, float* graph_pred_bias_in, int num_tasks);

/*
 * Replaces PNA_compute_graphs, PNA/src/dcl.h:91-111 (def. PNA/src/PNA_compute.cc:7-101).  No edge features.
 *   node_embedding_weight_in [S][173][80]
 *   node_conv_weights_in [S][4][80][3][4][80]  (layer, out, scaler {none,t,scale}, aggregator {mean,min,max,std}, in)
 *   node_conv_bias_in [S][4][80]
 *   graph_mlp_1_weights_in [S][40][80] / _bias [S][40];  graph_mlp_2 [S][20][40] / [S][20];  graph_mlp_3 [S][1][20] / [S][1]
 *   avg_deg_in [S]   (the reference host passes 6.885701656341553, PNA/src/host_load.cc:127)
 */
int PNA_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges,
                       int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in,
                       float* node_embedding_weight_in,
                       float* node_conv_weights_in, float* node_conv_bias_in,
                       float* graph_mlp_1_weights_in, float* graph_mlp_1_bias_in,
                       float* graph_mlp_2_weights_in, float* graph_mlp_2_bias_in,
                       float* graph_mlp_3_weights_in, float* graph_mlp_3_bias_in,
                       float* avg_deg_in);

/*
 * Replaces DGN_compute_graphs, DGN/src/dcl.h:71-91 (def. DGN/src/DGN_compute.cc:6-104).  No edge features.
 *   node_eigen_in float [N_tot][4]  (node_eigen_t, DGN/src/dcl.h:67; column 1 is the one used)
 *   embedding_h_atom_embedding_list_weights_in [S][9][119][100]  (dense per-feature tables)
 *   layers_posttrans_fully_connected_0_linear_weight_in [S][4][100][200] (= [out][2][in]) / _bias_in [S][4][100]
 *   MLP_layer_FC_layers_0 [S][50][100] / [S][50];  _1 [S][25][50] / [S][25];  _2 [S][1][25] / [S][1]
 */
int DGN_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges,
                       int* reload_weights, float* out,
                       int* node_feature_in, float* node_eigen_in, int* edge_list_in,
                       float* embedding_h_atom_embedding_list_weights_in,
                       float* layers_posttrans_fully_connected_0_linear_weight_in,
                       float* layers_posttrans_fully_connected_0_linear_bias_in,
                       float* MLP_layer_FC_layers_0_weight_in, float* MLP_layer_FC_layers_0_bias_in,
                       float* MLP_layer_FC_layers_1_weight_in, float* MLP_layer_FC_layers_1_bias_in,
                       float* MLP_layer_FC_layers_2_weight_in, float* MLP_layer_FC_layers_2_bias_in);

/*
 * Replaces GAT_compute_graphs, GAT/src/dcl.h:78-94 (def. GAT/src/GAT_compute.cc:7-112).  No edge features; the
 * node features are used as raw numbers (GAT/src/load_inputs.cc:190-191).
 *   scoring_fn_target_in / scoring_fn_source_in [S][5][4][16]
 *   linear_proj_weights_in / skip_proj_weights_in [S][5][4][16][4][16]  (layer, head_out, dim_out, head_in, dim_in);
 *       layer 0 uses only [head_out][dim_out][0][dim_in < 9] (GAT/src/host_load.cc:69-78)
 *   graph_pred_weights_in [S][1][16], graph_pred_bias_in [S][1]
 * Per-graph node-feature offsets ARE applied (the reference omits them, GAT_compute.cc:72); option
 * gat_reference_quirk = 1 (flowgnn_set_option / flowgnn_entry_set_option) reproduces the reference behaviour.
 */
int GAT_compute_graphs(int num_graphs, int* nums_of_nodes, int* nums_of_edges,
                       int* reload_weights, float* out,
                       int* node_feature_in, int* edge_list_in,
                       float* scoring_fn_target_in, float* scoring_fn_source_in,
                       float* linear_proj_weights_in, float* skip_proj_weights_in,
                       float* graph_pred_weights_in, float* graph_pred_bias_in);

/*
 * Devices and options of the entry points above (they have no handle to carry them).
 *  flowgnn_entry_set_devices: the HIP devices the six entry points run on.  With more than one, every run of constant weight
 *     set is cut into contiguous graph ranges balanced by sum(N + E) and the ranges run concurrently, one engine and one host
 *     thread per listed device (a device may be listed twice); `out` is filled in job order.  Default: device 0, or the list in
 *     the environment variable FLOWGNN_DEVICES (e.g. "0,1,2,3,4,5,6,7") read at the first call.
 *  flowgnn_entry_set_option: flowgnn_set_option for the engines behind the entry points of `model` (FLOWGNN_MODEL_*).
 *  flowgnn_entry_set_pipeline: the entry points take HOST arrays, so a large batch is cut into several ranges per engine and an
 *     engine's host -> device copy of its next range runs under the other engines' kernels (flowgnn_group_compute); with ONE listed
 *     device the entry points keep three engines on it for that.  0 (default): ranges of ~48 MB of host arrays, at most 8 per
 *     engine, small batches uncut on one engine; k >= 1: exactly k ranges per engine (1 = no pipelining, one engine per device).
 */
int flowgnn_entry_set_devices(int n_devices, const int* device_ids);
int flowgnn_entry_set_pipeline(int chunks_per_engine);
int flowgnn_entry_set_option(int model, const char* key, double value);
int flowgnn_entry_set_pooling(int model, int mode);       /* flowgnn_set_pooling (section 2) for the entry points of `model` */
int flowgnn_entry_set_gin_eps(int model, const float* eps); /* flowgnn_set_gin_eps (section 2): one vector for every weight set of the entry points; remembered for engines created later */

/* =====================================================================
 * (2) Handle API
 * ===================================================================== */
typedef struct flowgnn_engine flowgnn_engine;

/* Create an engine for `model` on HIP device `device_id`. */
int flowgnn_create(int model, int device_id, flowgnn_engine** out);
int flowgnn_destroy(flowgnn_engine* e);
/* Last HIP / IO error text for this engine (static storage, never NULL). */
const char* flowgnn_last_error(const flowgnn_engine* e);

/*
 * Weights, one weight set, host pointers, layouts as in the entry points above
 * without the leading [S].  Replaces the device-side load_weights
 * (GIN/src/load_inputs.cc:7-85).
 */
int flowgnn_set_weights_gin(flowgnn_engine* e,
                            const float* node_embedding_weight, const float* edge_embedding_weight,
                            const float* node_mlp_1_weights, const float* node_mlp_1_bias,
                            const float* node_mlp_2_weights, const float* node_mlp_2_bias,
                            const float* graph_pred_weights, const float* graph_pred_bias);

/*
 * Generic form: `count` host tensors of ONE weight set, in the argument order of the model's
 * <M>_compute_graphs entry point (GIN 8, GCN 11, GAT 6, PNA 10, DGN 9 tensors).
 */
int flowgnn_set_weights(flowgnn_engine* e, int count, const float* const* tensors);

/*
 * Read the reference's raw little-endian float32 .bin weight files from `dir`
 * (file names and offsets of <M>/src/host_load.cc; GIN: host_load.cc:24-58).
 */
int flowgnn_load_weights_dir(flowgnn_engine* e, const char* dir);

/*
 * Upload one concatenated batch (host pointers; copied to HBM, synchronous).
 * edge_attr may be NULL for models without edge features (GAT/PNA/DGN);
 * node_eigen ([N_tot][4] float, DGN/src/dcl.h:67) may be NULL except for DGN.
 * Replaces the host's flat-vector assembly + buffer migration
 * (GIN/src/host.cc:119-182).
 */
int flowgnn_set_batch(flowgnn_engine* e, int num_graphs,
                      const int* nums_of_nodes, const int* nums_of_edges,
                      const int* node_feature, const int* edge_list, const int* edge_attr,
                      const float* node_eigen);
/*
 * Upload one concatenated batch whose arrays are already in DEVICE memory of the engine's device (e.g. a PyG Batch moved to the
 * GPU, or a dataset kept in HBM), in one of two layouts:
 */
#define FLOWGNN_LAYOUT_REFERENCE 0  /* int32 arrays exactly as flowgnn_set_batch takes them: node_feature [N][9], edge_list [E][2] local ids, edge_attr [E][3] */
#define FLOWGNN_LAYOUT_PYG       1  /* int64 x [N][9], int64 edge_index [2][E] with batch-global node ids (PyG Batch), int64 edge_attr [E][3] */
/*
 *  nums_of_nodes / nums_of_edges are HOST arrays, as for flowgnn_set_batch: counts, offsets, limit checks, graph tiles,
 *  bin-packed tiles and the job totals / fill are built from them exactly as flowgnn_set_batch builds them, and the results are
 *  bit-identical to flowgnn_set_batch with the same arrays.  The edges of graph g are [eoff[g], eoff[g + 1]) (eoff = prefix sums of
 *  nums_of_edges), in both layouts: the order of a PyG Batch.  In the PyG layout an endpoint becomes local as id - noff[g]; an
 *  endpoint outside [noff[g], noff[g + 1]) or an int64 value that does not fit int32 becomes -1, which the device validation then
 *  refuses with the code flowgnn_set_batch would give (FLOWGNN_ERR_EDGE_RANGE / _EDGE_ATTR / _NODE_FEAT).  GAT reads its node
 *  features as raw numbers: there an x value outside int32 sets FLOWGNN_ERR_NODE_FEAT itself.  Such errors surface at
 *  flowgnn_sync / flowgnn_get_results, as validation errors do, and hold until the next set_batch.
 *  edge_attr may be NULL for GAT / PNA / DGN; node_eigen (float32 [N][4], both layouts) may be NULL except for DGN.
 *
 *  Asynchronous and stream-ordered: the ingest (PyG: one kernel that narrows, transposes and localises; reference: device-to-device
 *  copies) is enqueued on the engine's launch stream -- its own, or the one given to flowgnn_set_stream -- and the call does not
 *  wait for it; flowgnn_run needs no event to follow it.  The caller's arrays must be complete ON THAT STREAM when the call is made
 *  (order the stream after the producer's, e.g. with an event) and must stay unchanged until the ingest has run (a flowgnn_sync, or
 *  any later point on that stream).  The engine always copies into buffers of its own and keeps no pointer to the caller's.
 *
 *  Before anything is enqueued, every non-null array must be memory of the engine's device (hipPointerGetAttributes: pinned or
 *  pageable host memory is refused) and the bytes the counts imply must lie inside its allocation (hipMemGetAddressRange);
 *  otherwise, and for a NULL array the model needs or an unknown layout, FLOWGNN_ERR_ARG with a flowgnn_last_error text and no
 *  change to the engine.  Drops a recorded launch sequence (option hipgraph), as flowgnn_set_batch does.  Single engines only (a
 *  group's shards live on other devices).
 */
int flowgnn_set_batch_device(flowgnn_engine* e, int num_graphs,
                             const int* nums_of_nodes, const int* nums_of_edges,
                             int layout, const void* node_feature, const void* edge_list, const void* edge_attr,
                             const float* node_eigen);
/*
 * Declare the next flowgnn_set_batch batches to be SHARDS of a job of this many nodes and edges (a multi-process caller that cuts
 * one job over several GPUs, one engine each; flowgnn_group_* does it by itself).  The one choice between kernels that depends on the
 * batch size -- DGN's aggregation, by the density E / N (GIN's front end has had no size rule since round 4) -- is then made from
 * the job's totals, so every shard computes on the kernels a single engine would have chosen for the whole job and results do not
 * depend on the device count.  (-1, -1), the
 * default: each batch is its own job.  Totals smaller than a batch's own are raised to them.
 */
int flowgnn_set_job_totals(flowgnn_engine* e, long long job_nodes, long long job_edges);
/*
 * The other size-dependent choice: the graph-resident / fused kernels are used when the batch's graph tiles pack at least as full as
 * the model's threshold (GIN / GIN-VN: option "gin_resident_min_fill", default 50 %; GCN / GAT 50 %; PNA / DGN 40 %; the last tile does
 * not count).  flowgnn_graph_tile_fill computes that fill for any graph list under this engine's
 * model and options (host code, no device work; -1: the model has no graph tiles, 0: a graph exceeds the tile limits);
 * flowgnn_set_job_tile_fill makes the next flowgnn_set_batch batches take the side of the threshold the JOB's fill is on, whatever
 * their own graphs pack to (< 0: back to each batch's own packing).  flowgnn_group_* and the entry points hand both down by themselves.
 * (Development builds only -- make DEV=1, option "gin_pingpong": that kernel decides by the SHARD's own half-tile fill, which is not
 * handed down; the shipped library has no such path.)
 */
int flowgnn_graph_tile_fill(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, double* fill);
int flowgnn_set_job_tile_fill(flowgnn_engine* e, double fill);

/*
 * Enqueue one full forward of the resident batch on the engine's stream:
 * batched load_graph (CSR by destination) -> atom encoder -> conv layers ->
 * readout.  Asynchronous; results land in the engine's device result buffer.
 * Replaces one enqueueTask of <M>_compute_graphs (GIN/src/host.cc:203-210).
 */
int flowgnn_run(flowgnn_engine* e);
/* Wait for the engine's stream; returns the first validation / HIP error seen. */
int flowgnn_sync(flowgnn_engine* e);
/* Copy results [num_graphs] to host (synchronises the stream first). */
int flowgnn_get_results(flowgnn_engine* e, float* out_host);
/* Device pointer of the result buffer (float[num_graphs]); valid until next set_batch. */
int flowgnn_results_device(flowgnn_engine* e, void** d_out);
/*
 * Redirect results into a caller-owned DEVICE buffer of at least num_graphs floats (e.g. a
 * torch tensor's data_ptr(), so RCCL can all-gather it without a copy); NULL restores the
 * engine's own buffer.  Applies to the resident batch and is reset by flowgnn_set_batch.  Does not wait for the device: it
 * affects the runs enqueued after it (a caller alternating two buffers from step to step pays no host synchronisation).
 */
int flowgnn_set_results_buffer(flowgnn_engine* e, void* device_ptr);
/*
 * Graph embeddings: beside the logits, the vector the model's readout head is applied to,
 *     emb[g][:] = (1 / n_g) * sum over the nodes v of graph g of r[v][:]          (fp32, [num_graphs][flowgnn_embedding_dim(model)])
 * with r = the rows the readout pools, so that head(emb[g]) is the graph's logit:
 *     GIN, GIN-VN  h_5, the last layer's output (no ReLU after it)                               100
 *     GCN          BatchNorm_4(aggregation of x_4), no ReLU                                      100
 *     GAT          the last layer's output averaged over its 4 heads                              16
 *     PNA          h_4                                                                            80
 *     DGN          h_4                                                                           100
 * and n_g the node count the readout divides by (GIN-VN: the virtual node counts, as in its logit).  A graph's rows are summed in
 * an order that depends on the graph alone, so embeddings -- like the logits -- are bit-identical under batch order, slices and
 * group cuts wherever the paragraph above flowgnn_group promises that of the logits.
 *  flowgnn_embedding_dim: floats per graph (-1: unknown model).  Needs no GPU.
 *  flowgnn_set_embeddings(e, 1): the runs enqueued after it also produce the embeddings.  Off by default, and off means off: the
 *     same kernels launch with the same arguments and every result bit is what it was.  On, PNA and DGN run the instance of their
 *     kernels that also stores the pooled row the readout forms anyway (logits bit-identical to off); GIN / GIN-VN run the
 *     graph-resident kernel's UN-FOLDED
 *     instance, which pools h_5 out of on-chip memory -- their logits are then those of the un-folded rule, which differ from the
 *     default folded ones by fp32 rounding (FLOWGNN_NUMERIC_F16: by the "every other path" rule of that mode, and the embedding is
 *     the pooled h_5 = f16(W2) f16(hidden) + b2 of that rule); GCN and GAT leave their graph-resident kernels for the per-layer
 *     path with the un-folded last stage (same rule for their logits), which costs them their on-chip speed: DESIGN.md.
 *     FLOWGNN_ERR_UNSUPPORTED in FLOWGNN_NUMERIC_Q6_10 (there are no fixed-point embeddings), and flowgnn_set_numeric_mode
 *     answers the same for that mode while embeddings are on.  Drops a recorded launch sequence (option hipgraph).  Survives
 *     flowgnn_set_batch.  The <M>_compute_graphs entry points never produce embeddings.
 *  flowgnn_get_embeddings: copy [num_graphs][dim] to the host (synchronises first, like flowgnn_get_results; an exact-fp32
 *     re-run refills the embeddings with the logits).  FLOWGNN_ERR_STATE when the last run did not have embeddings on.
 *  flowgnn_embeddings_device: where the last run put them (same condition); valid until the next flowgnn_set_batch.
 *  flowgnn_set_embeddings_buffer: redirect them into a caller-owned DEVICE buffer of at least num_graphs * dim floats, as
 *     flowgnn_set_results_buffer does for the logits; NULL restores the engine's own buffer; reset by flowgnn_set_batch; drops a
 *     recorded launch sequence.
 */
int flowgnn_embedding_dim(int model);
int flowgnn_set_embeddings(flowgnn_engine* e, int on);
int flowgnn_get_embeddings(flowgnn_engine* e, float* out_host);
int flowgnn_embeddings_device(flowgnn_engine* e, void** d_emb);
int flowgnn_set_embeddings_buffer(flowgnn_engine* e, void* device_ptr);

/*
 * Node embeddings: the rows that pool is taken over, one per node,
 *     node_emb[v][:] = r[v][:]                                                     (fp32, [N_tot][flowgnn_embedding_dim(model)])
 * with r as defined above (GIN / GIN-VN h_5 without ReLU, GCN BatchNorm_4(aggregation of x_4) without ReLU, GAT the last layer's
 * output averaged over its 4 heads, PNA / DGN h_4) and v the node's position in the batch AS THE CALLER PASSED IT, whatever order
 * the bin-packed tiles walk the graphs in.  GIN-VN: the virtual nodes are rows like any other.  mean over a graph's rows = emb[g],
 * and head(emb[g]) = the graph's logit.  What a pooling of the caller's own, a node-level head or an attribution reads.
 *  flowgnn_set_node_embeddings(e, 1): the runs enqueued after it also store the rows.  Off by default, and off means off: the same
 *     kernels launch with the same arguments and every result bit is what it was.  The logits while it is on:
 *       GCN, PNA, DGN   bit-identical to off.  Where the batch runs on the graph-resident kernel it stays there: the instance
 *                       gcn_resident_rows_kernel / pna_resident_rows_kernel / dgn_resident_rows_kernel keeps its folded / pooled
 *                       readout and additionally stores the rows it holds on chip at the end of the last layer;
 *       GIN, GIN-VN     those of the un-folded rule, exactly as documented for flowgnn_set_embeddings (FLOWGNN_NUMERIC_F16: the
 *                       "every other path" rule of that mode): the graph-resident kernel's un-folded instance writes h_5;
 *       GAT             those of its un-folded per-layer path, as with flowgnn_set_embeddings: gat_resident_kernel folds the last
 *                       layer's skip contraction into the readout and never forms the 16-wide row (the open item).
 *     The per-layer paths (options <model>_resident 0, batches under the fill threshold, graphs beyond the tile limits) and the
 *     exact-fp32 re-run fill the buffer from the rows they keep in HBM, with the last stage un-folded.
 *     FLOWGNN_ERR_UNSUPPORTED in FLOWGNN_NUMERIC_Q6_10, and flowgnn_set_numeric_mode answers the same for that mode while node
 *     embeddings are on.  Drops a recorded launch sequence (option hipgraph).  Survives flowgnn_set_batch.  Works together with
 *     flowgnn_set_embeddings, NUM_TASK > 1, FLOWGNN_NUMERIC_F16 and option hipgraph.  The <M>_compute_graphs entry points never
 *     produce rows.
 *  flowgnn_get_node_embeddings: copy [N_tot][dim] to the host (synchronises first; an exact-fp32 re-run refills the rows with the
 *     logits).  FLOWGNN_ERR_STATE when the last run did not have node embeddings on.
 *  flowgnn_node_embeddings_device: where the last run put them (same condition); valid until the next flowgnn_set_batch.
 *  flowgnn_set_node_embeddings_buffer: redirect them into a caller-owned DEVICE buffer of at least N_tot * dim floats; NULL
 *     restores the engine's own buffer; reset by flowgnn_set_batch; drops a recorded launch sequence.  The engine writes only into
 *     its own buffer or this one, on its stream: a stream-ordered caller needs no host synchronisation.
 */
int flowgnn_set_node_embeddings(flowgnn_engine* e, int on);
int flowgnn_get_node_embeddings(flowgnn_engine* e, float* out_host);
int flowgnn_node_embeddings_device(flowgnn_engine* e, void** d_rows);
int flowgnn_set_node_embeddings_buffer(flowgnn_engine* e, void* device_ptr);

/*
 * Node logits (GIN, GIN-VN, GCN, GAT): these four models read out with a mean pool and a linear head, so a graph's logit is the
 * mean of one number per node,
 *     node_logit[v][t] = r[v] . W[t] + b[t]                                         (fp32, [N_tot][NUM_TASK])
 *     logit[g][t]      = (1 / n_g) * sum over the nodes v of g of node_logit[v][t]
 * with r[v] the row flowgnn_set_node_embeddings returns, W / b the head, and v the node's position in the batch AS THE CALLER
 * PASSED IT (GIN-VN: the virtual nodes are nodes).  An exact additive attribution of a graph's prediction to its nodes, and a
 * per-node output for node-level use -- 4 bytes per node and task where the row is 64 or 400.
 *  flowgnn_set_node_logits(e, 1): the runs enqueued after it also store the terms.  Off by default, and off means off: the same
 *     kernels launch with the same arguments.  While it is on, alone, the batch stays on the kernels it runs on with it off and
 *     the graph logits keep their bits: on the graph-resident path the instances gin_resident_nlogit_kernel /
 *     gcn_resident_nlogit_kernel / gat_resident_nlogit_kernel are the default kernels plus one 4-byte store per node of the term
 *     they hold in LDS anyway (GAT included: it keeps its graph-resident launch); the folded per-layer paths add the constant to
 *     the per-node scores they leave in device memory; wherever the rows themselves are in device memory (un-folded paths,
 *     NUM_TASK > 1, the exact-fp32 re-run, graph or node embeddings on as well) one small kernel takes rows[v] . W[t] + b[t], a
 *     fixed summation order per value.  No atomics anywhere.
 *     FLOWGNN_ERR_UNSUPPORTED for PNA and DGN: they read the pooled vector through an MLP head, so no such decomposition exists.
 *     FLOWGNN_ERR_UNSUPPORTED in FLOWGNN_NUMERIC_Q6_10, and flowgnn_set_numeric_mode answers the same for that mode while node
 *     logits are on.  Drops a recorded launch sequence (option hipgraph).  Survives flowgnn_set_batch.  Works together with
 *     flowgnn_set_embeddings, flowgnn_set_node_embeddings, NUM_TASK > 1, FLOWGNN_NUMERIC_F16 (GIN / GIN-VN) and option hipgraph.
 *     The <M>_compute_graphs entry points never produce them.
 *  flowgnn_get_node_logits: copy [N_tot][NUM_TASK] to the host (synchronises first; an exact-fp32 re-run refills them with the
 *     logits).  FLOWGNN_ERR_STATE when the last run did not have node logits on.
 *  flowgnn_node_logits_device: where the last run put them (same condition); valid until the next flowgnn_set_batch.
 *  flowgnn_set_node_logits_buffer: redirect them into a caller-owned DEVICE buffer of at least N_tot * NUM_TASK floats; NULL
 *     restores the engine's own buffer; reset by flowgnn_set_batch; drops a recorded launch sequence.
 */
int flowgnn_set_node_logits(flowgnn_engine* e, int on);
int flowgnn_get_node_logits(flowgnn_engine* e, float* out_host);
int flowgnn_node_logits_device(flowgnn_engine* e, void** d_terms);
int flowgnn_set_node_logits_buffer(flowgnn_engine* e, void* device_ptr);

/*
 * Attention coefficients (GAT): what PyG's GATConv(return_attention_weights=True) returns, for explanation and edge pruning.
 * For layer l (0..4), head h (0..3) and destination v, with the reference's implicit self edge first:
 *     e(u->v)[l][h]       = exp(leaky_0.2(ssrc_l[v][h] + stgt_l[u][h]))                  (no max subtraction, as the reference)
 *     den[v][l][h]        = e(v->v) + sum over the in-edges (u->v) of e(u->v)
 *     attn_edge[l][i][h]  = e(u_i->v_i) / den[v_i]     for edge i of the batch AS THE CALLER PASSED IT
 *     attn_self[l][v][h]  = e(v->v) / den[v]           for node v in the caller's node order
 * An explicit [v, v] entry of the edge list is an ordinary edge beside the self term; duplicate edges each get their own (equal)
 * value.  fp32, and the very coefficients the kernel's message is formed with (the same e, the same 1 / den).  Outputs are
 * layer-major over the SELECTED layers only, in ascending layer order: attn_edge [n_sel][E_tot][4], attn_self [n_sel][N_tot][4].
 *  flowgnn_attention_shape: layers = 5, heads = 4 for GAT; FLOWGNN_ERR_UNSUPPORTED for every other model.  Needs no GPU.
 *  flowgnn_set_attention(e, layer_mask): bit l selects layer l, n_sel = popcount(mask), 0 = off (the default); 16 is the last layer,
 *     what the common uses want -- all five layers are 80 bytes per edge and node.  Off means off: the same kernels launch with
 *     the same arguments.  On, alone, the batch stays on the kernels it runs on with it off and the graph logits keep their bits:
 *     the graph-resident path launches gat_resident_attn_kernel (gat_attn.hip: the default kernel, which in the selected layers
 *     parks every edge's e in LDS during its walk and stores e * rcp(den) when the walk has formed den -- by the lane that walked
 *     the row, edge values through the index build's edge ids, no atomics; it stores the node logits as well when those are on).
 *     Every other path (gat_resident 0, batches under the fill threshold, graphs beyond 256 rows / 1 280 in-edges, the exact-fp32
 *     re-run, graph or node embeddings on) launches gat_attention_kernel beside each selected layer: a lane per destination, the
 *     row's CSR order, e / den.  The two paths may differ by fp32 rounding (exp2 of pre-scaled scores and a reciprocal against
 *     expf and a division), as their logits do; neither depends on tile placement or on the order of the caller's edge list.
 *     FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why) for a non-zero mask on any other model, and in FLOWGNN_NUMERIC_Q6_10;
 *     flowgnn_set_numeric_mode answers the same for that mode while attention is on.  FLOWGNN_ERR_ARG for a mask outside 0..31.
 *     Drops a recorded launch sequence (option hipgraph).  Survives flowgnn_set_batch.  Works together with
 *     flowgnn_set_embeddings, flowgnn_set_node_embeddings, flowgnn_set_node_logits, option hipgraph, gat_reference_quirk and
 *     flowgnn_set_batch_device.  The <M>_compute_graphs entry points never produce them.
 *  flowgnn_get_attention: copy to the host (either pointer may be NULL; synchronises first; an exact-fp32 re-run refills the values
 *     with the logits).  FLOWGNN_ERR_STATE when the last run had attention off, or on with another mask than the current one.
 *  flowgnn_attention_device: where the last run put them (same condition; either pointer may be NULL); valid until the next
 *     flowgnn_set_batch.
 *  flowgnn_set_attention_buffers: redirect them into caller-owned DEVICE buffers of at least n_sel * E_tot * 4 and n_sel * N_tot * 4
 *     floats; NULL restores the engine's own buffer (each of the two on its own); reset by flowgnn_set_batch; drops a recorded
 *     launch sequence; stream-ordered, no host synchronisation.
 */
int flowgnn_attention_shape(int model, int* layers, int* heads);
int flowgnn_set_attention(flowgnn_engine* e, int layer_mask);
int flowgnn_get_attention(flowgnn_engine* e, float* edge_host, float* self_host);
int flowgnn_attention_device(flowgnn_engine* e, void** d_edge, void** d_self);
int flowgnn_set_attention_buffers(flowgnn_engine* e, void* d_edge, void* d_self);

/* The engine's hipStream_t as an opaque pointer (for event timing by a caller). */
int flowgnn_stream(flowgnn_engine* e, void** stream);

/*
 * Make the engine launch on a caller-owned hipStream_t (use_external != 0; `stream` may be the null stream) instead of
 * its own, e.g. the stream a collective library orders itself against, so that "forward, then all-gather the results"
 * needs no host synchronisation in between.  use_external == 0 restores the engine's own stream.  The caller keeps
 * the stream alive for as long as the engine uses it.
 */
int flowgnn_set_stream(flowgnn_engine* e, void* stream, int use_external);

/* Totals of the resident batch. */
int flowgnn_batch_info(const flowgnn_engine* e, long long* num_graphs,
                       long long* total_nodes, long long* total_edges);
/*
 * Graph tiles of the resident batch (0, 0 when the model keeps no whole graphs on chip or a graph exceeds its tile limits):
 * *batch_order = tiles cut in batch order (what the per-layer kernels and taps use), *packed = the bin-packed tile lists a
 * graph-resident kernel walks instead when the model asks for them (options <model>_binpack; 0 = not built).
 */
int flowgnn_batch_tiles(const flowgnn_engine* e, int* batch_order, int* packed);

/*
 * Number of forward passes this engine repeated on its exact-fp32 kernels because
 * an operand left the range in which the default kernels are fp32-accurate (GIN:
 * the dense update runs as three f16 MFMAs per product, accurate to 2^-20 relative
 * while 6e-5 < |activation| < 6e4 and to 6e-8 ABSOLUTE per operand below that -- no
 * flag is raised for tiny operands; the reference's own Q6.10 activations live in
 * [-32,32) on a 2^-10 grid).
 * The check happens in flowgnn_sync / flowgnn_get_results: device-side consumers
 * of flowgnn_results_device must call flowgnn_sync first.  -1 for a null handle.
 */
int flowgnn_exact_reruns(const flowgnn_engine* e);

/*
 * Launch-sequence replay (opt-in: option hipgraph = 1 for resident batches of up to 2^20 nodes, 2 for any size).
 * flowgnn_run then records its launch sequence (index build + forward pass) into a hipGraph on the second run of a
 * batch and replays it afterwards; any call that changes what the kernels read or write (weights, batch, result
 * buffer, numeric mode, an exact-fp32 re-run) drops the recording, and runs with the profiler enabled are never
 * replays.  Off by default: on the measured runtime plain asynchronous launches are as fast (NOTEBOOK.md section 5).
 * Returns how many runs of this engine were replays (-1 for a null handle).
 */
long long flowgnn_graph_replays(const flowgnn_engine* e);

/*
 * NUM_TASK of the readout as a run-time dimension (a compile-time constant in the reference, GIN/src/dcl.h:25, 1 as
 * shipped; ogbg-molpcba has 128 tasks).  graph_pred_weights is then [NUM_TASK][EMB_DIM], graph_pred_bias [NUM_TASK], and
 * the results are [num_graphs][NUM_TASK] (out[g][t], as `FM_TYPE out[][NUM_TASK]`, GIN/src/dcl.h:80) -- every buffer that
 * receives results (flowgnn_get_results, flowgnn_set_results_buffer) holds num_graphs * NUM_TASK floats.  Call it before
 * setting weights and batch (both must be set again afterwards).  GIN / GIN-VN / GCN; the other models' readouts are
 * single-task MLP heads and return FLOWGNN_ERR_UNSUPPORTED for NUM_TASK != 1.  The entry points take NUM_TASK as an explicit
 * argument (GIN_compute_graphs_mt / GCN_compute_graphs_mt).
 */
int flowgnn_set_num_tasks(flowgnn_engine* e, int num_tasks);
int flowgnn_num_tasks(const flowgnn_engine* e);

/*
 * EMB_DIM of GIN as a run-time choice between two widths (a compile-time constant in the reference, GIN/src/dcl.h:19, 100 as
 * shipped; OGB's own training script defaults to --emb_dim 300, and the GIN results quoted for ogbg-molhiv / ogbg-molpcba are
 * 300-wide models).  At FLOWGNN_EMB_DIM_OGB the eight GIN tensors are node_emb [173][300], edge_emb [5][13][300], w1 [5][600][300],
 * b1 [5][600], w2 [5][300][600], b2 [5][300], pred_w [NUM_TASK][300], pred_b [NUM_TASK] (every leading 5 is flowgnn_num_layers(e),
 * which flowgnn_set_num_layers below changes at this width); flowgnn_load_weights_dir reads the
 * reference's file names with dim300 in place of dim100; embeddings, node embeddings and flowgnn_get_h are 300 wide.  The width runs
 * on kernels of its own, one launch per layer: split-f16 MFMA products with the fp32 re-run of flowgnn_exact_reruns.
 * Call it before setting weights and batch (both must be set again afterwards: weights set before are dropped); drops a recorded
 * launch sequence; setting the width the engine has is a no-op.  FLOWGNN_MODEL_GIN only: every other model, GIN-VN included, returns
 * FLOWGNN_ERR_UNSUPPORTED (GCN's width goes through flowgnn_set_model_emb_dim below, and the error text says so).  At 300, FLOWGNN_NUMERIC_Q6_10 / FLOWGNN_NUMERIC_F16 through flowgnn_set_numeric_mode (F16 at
 * that width goes through flowgnn_set_numeric_mode_dim), flowgnn_set_ogb_virtual_node (its tensors are 100
 * wide; 300-wide ones go through flowgnn_set_ogb_virtual_node_dim) and flowgnn_run_aggregation_only / flowgnn_get_aggregate return FLOWGNN_ERR_UNSUPPORTED, and so does this call while one
 * of the first three is on.  A width other than the two: FLOWGNN_ERR_ARG.  flowgnn_embedding_dim(model) keeps answering for the
 * model's default width; flowgnn_emb_dim(e) is the engine's (-1 for a null handle).  The <M>_compute_graphs entry points have no
 * 300-wide form.
 */
#define FLOWGNN_EMB_DIM_REFERENCE 100
#define FLOWGNN_EMB_DIM_OGB       300
/* PNA's own width, flowgnn_embedding_dim(FLOWGNN_MODEL_PNA): no choice of width, but the argument that flowgnn_set_model_numeric_mode_dim
 * takes on a FLOWGNN_MODEL_PNA engine (below). */
#define FLOWGNN_EMB_DIM_PNA       80
int flowgnn_set_emb_dim(flowgnn_engine* e, int emb_dim);   /* 100 (default) or 300 */
int flowgnn_emb_dim(const flowgnn_engine* e);              /* -1 for a null handle */

/*
 * The width of GIN or GCN: the call that names no model.  On a GIN engine it is exactly flowgnn_set_emb_dim (the same code path, state
 * and bits).  On a GCN engine it chooses between the reference's width and OGB's default, the width of a GNN(gnn_type='gcn')
 * checkpoint trained with OGB's own script: at FLOWGNN_EMB_DIM_OGB the eleven GCN tensors are node_emb [173][300], edge_emb
 * [5][13][300], convs_weight [5][300][300], convs_bias / root_emb / bn_weight / bn_bias / bn_mean / bn_var [5][300], pred_w
 * [NUM_TASK][300], pred_b [NUM_TASK] (every leading 5 is flowgnn_num_layers(e), flowgnn_set_num_layers below); flowgnn_load_weights_dir reads gcn_ep1_dim300.weights.all.bin, the reference's one file with
 * 300 for 100 in every offset; embeddings, node embeddings and flowgnn_get_h (the rows the readout pools) are 300 wide.  The width
 * runs on kernels of its own (gcn_wide.hip): one fused launch per layer with split-f16 MFMA products and the fp32
 * re-run of flowgnn_exact_reruns.  NUM_TASK, the three poolings, graph embeddings, node embeddings, node logits, host and device
 * batches and groups work as at 100.  flowgnn_set_option values that choose among the 100-wide GCN paths (gcn_resident, gcn_binpack,
 * gcn_tile_build, gcn_unfused, gcn_mfma) are accepted and have no effect at 300.
 * The same sequence as flowgnn_set_emb_dim: weights and batch must be set again after a change, and the width the engine has is a
 * no-op.  Any other model: FLOWGNN_ERR_UNSUPPORTED; a width other than the two: FLOWGNN_ERR_ARG.  On a GCN engine at 300,
 * FLOWGNN_NUMERIC_Q6_10, flowgnn_set_gcn_virtual_node with tensors (they are 100 wide; 300-wide ones go through
 * flowgnn_set_gcn_virtual_node_dim; all five NULL stays accepted), flowgnn_run_aggregation_only and flowgnn_get_aggregate return
 * FLOWGNN_ERR_UNSUPPORTED, and so does this call while the fixed-point mode or GCN's virtual node of the other width is on.  flowgnn_set_emb_dim on a GCN engine stays FLOWGNN_ERR_UNSUPPORTED and
 * names this call.  flowgnn_embedding_dim(FLOWGNN_MODEL_GCN) stays 100.
 * Where the engine's GCN is OGB's GCNConv (either width): on batches that list both directions of every edge, as every OGB molecule
 * dataset does.  The engine follows the reference, whose normalisation is 0 at a node without out-edges; OGB takes
 * (out-degree + 1)^-1/2 there, so a message into such a node is dropped here and delivered there.
 */
int flowgnn_set_model_emb_dim(flowgnn_engine* e, int emb_dim);   /* GIN, GCN: 100 (default) or 300 */

/*
 * Numeric mode of the engine.  FLOWGNN_NUMERIC_F32 (default): fp32 storage and accumulation.
 * FLOWGNN_NUMERIC_Q6_10: every value is the bit pattern of the reference's own number format -- ap_fixed<16,6> for GIN,
 * GIN-VN, GCN, GAT and PNA (GIN/src/dcl.h:58-59: 10 fractional bits, truncation toward -inf, wrap on overflow), ap_fixed<16,3>
 * for DGN (DGN/src/dcl.h:54-55: 13 fractional bits) -- weights are quantised from the float tensors as the reference host
 * does, and the outputs are pattern / 2^F (exact in float).  The rules assumed for ap_fixed division and the hls:: math
 * functions are written down in oracle/ginq_oracle.c and oracle/q_oracle.c.  A fidelity mode, one to two orders of
 * magnitude slower than the default path: products are truncated one at a time, as the reference does.
 * NOT validated against Vitis: the rules are taken from the published ap_fixed / hls_math semantics and the tests prove that
 * the GPU kernels and the CPU restatement agree bit for bit with EACH OTHER; no Vitis header or C-simulation output exists in
 * this repository's build environment to pin them to the reference's real bit patterns.
 */
#define FLOWGNN_NUMERIC_F32 0
#define FLOWGNN_NUMERIC_Q6_10 1
/*
 * FLOWGNN_NUMERIC_F16 (through this call: GIN and GIN-VN only, NUM_TASK 1 or more; every other model returns FLOWGNN_ERR_UNSUPPORTED --
 * GIN and GCN at width 300 and PNA have theirs behind flowgnn_set_numeric_mode_dim / flowgnn_set_model_numeric_mode_dim below, DGN
 * behind flowgnn_set_model_numeric_mode, the call that names the model and reaches every mode any engine has): the
 * 16-bit operand speed of the matrix pipe.  Every operand of the node MLP's two linear layers -- the weights and the
 * activation each of them multiplies -- is rounded to f16 (round to nearest even), and each product is ONE f16 x f16 MFMA
 * with fp32 accumulation (the default mode forms every product from three).  The weights are rounded after the exact
 * power-of-two scale the kernels apply per matrix: the same values as rounding the weights themselves unless an entry
 * falls below the f16 normal range (6.1e-5 times the matrix's largest entry).  fp32 as in the default mode: the atom
 * encoder, the in-edge walk and its sums, biases, BatchNorm (folded into the weights as in the default mode), the ReLUs,
 * the mean pool and the readout's dot product.  Where the readout rounds:
 *   - single-task, graph-resident path (the default for molecule-sized graphs): the readout is folded through the last
 *     layer's second linear layer, logit = mean_v(f16(hidden_v) . f16(u)) + b2 . w_pred + b, with u = W2^T w_pred
 *     rounded to f16 once;
 *   - every other path (NUM_TASK > 1, the per-layer kernels of option gin_resident 0 and of batches the resident kernel
 *     does not take, flowgnn_get_h taps): h_5 = W2 f16(hidden) + b2 with f16(W2), then the fp32 readout of h_5.
 * Range fallback as in the default mode: an MLP operand beyond the f16 range (|x| > 6e4) raises the range flag and the
 * forward pass is repeated on the fp32 kernels -- that batch's results are then f32-mode results (flowgnn_exact_reruns
 * counts it).  Options that select non-split kernels (gin_mfma 32, gin_unfused 1) give f32-mode results in this mode.
 * Within one path results are bit-identical under batch order, slices and group cuts, as in the default mode.  The
 * reference-compatible <M>_compute_graphs entry points keep the default mode.  Switch before or after setting weights.
 */
#define FLOWGNN_NUMERIC_F16 2
int flowgnn_set_numeric_mode(flowgnn_engine* e, int mode);
/*
 * The numeric mode with the width it is meant for: emb_dim must be the engine's width (FLOWGNN_ERR_ARG otherwise, the text names both
 * numbers; also for a width that is neither 100 nor 300 and for an unknown mode).  With emb_dim FLOWGNN_EMB_DIM_REFERENCE the call IS
 * flowgnn_set_numeric_mode.  With FLOWGNN_EMB_DIM_OGB, on a FLOWGNN_MODEL_GIN engine at that width (flowgnn_set_emb_dim), it accepts
 * FLOWGNN_NUMERIC_F32 and FLOWGNN_NUMERIC_F16; FLOWGNN_NUMERIC_Q6_10, and any mode but F32 on a GCN engine at that width, return
 * FLOWGNN_ERR_UNSUPPORTED.  flowgnn_set_numeric_mode itself keeps answering FLOWGNN_ERR_UNSUPPORTED to every mode but F32 at width 300.
 * FLOWGNN_NUMERIC_F16 at width 300, with D = 300, H = 600, the un-folded rule of the text above:
 *   a[v] = fma(h[v], s_l, sum_e relu(h[src_e] + ecomb_l[code_e])) in fp32, in CSR order, as in the default mode; then a, the ReLU'd
 *   hidden units (in the kernels' scaled domain, r(hid s1) / s1) and both weight matrices after their power-of-two scale (r(W s) / s)
 *   are rounded to f16, to nearest even, and each product is ONE f16 x f16 MFMA with fp32 accumulation; biases and 1 / (s1 s2) as in
 *   the default mode.  fp32 and unchanged: the encoder, the walk, eps, OGB's virtual node (only the node MLP's operands are rounded;
 *   the virtual node's add and its update MLP are the default mode's), the pooling, the attention readout's gate, the head and the
 *   node logits.  Range fallback as above: beyond 6e4 the pass is repeated on the fp32 kernels of the default mode's exact path.
 * The mode is the engine's: it survives flowgnn_set_weights, new batches, eps, pooling, NUM_TASK and the virtual-node and attention
 * readout setters, in either order with them.  While it is not FLOWGNN_NUMERIC_F32 at width 300, flowgnn_set_emb_dim /
 * flowgnn_set_model_emb_dim to width 100 return FLOWGNN_ERR_UNSUPPORTED (set F32, change the width, set the mode again); the same
 * width again stays a no-op.
 */
int flowgnn_set_numeric_mode_dim(flowgnn_engine* e, int emb_dim, int mode);
/*
 * The same call in the form that names no model, as flowgnn_set_model_emb_dim is for the width.  On a FLOWGNN_MODEL_GIN engine it IS
 * flowgnn_set_numeric_mode_dim; at emb_dim FLOWGNN_EMB_DIM_REFERENCE on any engine it IS flowgnn_set_numeric_mode (GCN's F16 at width
 * 100 stays FLOWGNN_ERR_UNSUPPORTED).  On a FLOWGNN_MODEL_GCN engine at FLOWGNN_EMB_DIM_OGB (flowgnn_set_model_emb_dim) it accepts
 * FLOWGNN_NUMERIC_F32 and FLOWGNN_NUMERIC_F16; FLOWGNN_NUMERIC_Q6_10 returns FLOWGNN_ERR_UNSUPPORTED.  emb_dim other than the engine's
 * width, a width that is neither 100 nor 300, an unknown mode and a null handle: FLOWGNN_ERR_ARG, as above.  flowgnn_set_numeric_mode
 * and flowgnn_set_numeric_mode_dim keep answering FLOWGNN_ERR_UNSUPPORTED to F16 on a GCN engine at width 300; their texts name this call.
 * FLOWGNN_NUMERIC_F16 for GCN / gcn-virtual at width 300, with D = 300: in stages s = 0..3 the two operands of
 * the layer's one product x_{s+1} = W_{s+1} a_{s+1} + b_{s+1} are rounded to f16, to nearest even --
 *   a_{s+1}, what the kernel holds behind the walk, the epilogue (root, 1 / (deg + 1), the folded BatchNorm, ReLU), the residual add and
 *   the virtual node's add, at the point where the default mode splits it into two halves;
 *   the weight matrix after its power-of-two scale, r(W s) / s: the hi halves of the default mode's split stream
 * -- and the product is ONE f16 x f16 MFMA per K-step and output tile, with fp32 accumulation, the pre-scaled bias and 1 / s as in the
 * default mode.  fp32 and unchanged: the encoder and x_0, the walk, root, 1 / (deg + 1) and the folded BatchNorm, the residual add and the
 * virtual node's add, the partial rows and the rows of flowgnn_set_model_jk_residual (they hold the unrounded a), stage 4, the virtual
 * node's sums and its update MLP, the pools, every readout (mean, sum, max, attention, set2set), the head and the node logits.  Range
 * fallback as above: a beyond 6e4 raises the flag and the pass is repeated on the default mode's exact fp32 path.
 * The mode is the engine's: it survives flowgnn_set_weights, new batches, pooling, NUM_TASK, flowgnn_set_gcn_virtual_node_dim,
 * flowgnn_set_model_jk_residual and the attention and set2set readout setters, in either order with them.  While it is not
 * FLOWGNN_NUMERIC_F32, flowgnn_set_model_emb_dim(e, 100) returns FLOWGNN_ERR_UNSUPPORTED and leaves the mode as it was (set F32, change
 * the width, set the mode again); the same width again stays a no-op.  flowgnn_set_numeric_mode(e, FLOWGNN_NUMERIC_F32) always goes back.
 */
int flowgnn_set_model_numeric_mode_dim(flowgnn_engine* e, int emb_dim, int mode);
/*
 * flowgnn_set_model_numeric_mode_dim on a FLOWGNN_MODEL_PNA engine: the call above also takes the model's true width, FLOWGNN_EMB_DIM_PNA (80, what
 * flowgnn_embedding_dim(FLOWGNN_MODEL_PNA) returns), and there it accepts FLOWGNN_NUMERIC_F32, FLOWGNN_NUMERIC_Q6_10 (both as
 * flowgnn_set_numeric_mode has them) and FLOWGNN_NUMERIC_F16: the one way to PNA's f16 mode.  Every other call keeps its answer on a
 * PNA engine -- flowgnn_set_numeric_mode, flowgnn_set_numeric_mode_dim and this call at emb_dim 100 return FLOWGNN_ERR_UNSUPPORTED for
 * F16, and the text names this form; flowgnn_set_numeric_mode_dim(e, 80, ..) is FLOWGNN_ERR_ARG, and its text names this form too.  On
 * every other engine emb_dim 80 stays FLOWGNN_ERR_ARG.
 * FLOWGNN_NUMERIC_F16 for PNA changes the layer's 320 -> 3 x 80 contraction and nothing else:
 *   each of a node's 320 aggregates (mean, min, max, std of 80 features, as the walk forms them in fp32 -- the sentinels
 *   31.9990234375 and -32 of a row without in-edges included: the first rounds to 32) is rounded to f16 ONCE, to nearest even, at the
 *   point where the default mode splits it into two halves; the conv weights are rounded after the layer's power-of-two scale, r(W s);
 *   each product is ONE f16 x f16 MFMA with fp32 accumulation, in the default mode's accumulator order.
 * fp32 and unchanged: the encoder sum, the walk (sums, squares, min, max, 1 / indeg, the square root), the scalers t and scale and the
 * update h + relu(b + Y_0 + t Y_1 + scale Y_2), the rows (on chip and in HBM), the mean pool and the 80 -> 40 -> 20 -> 1 head.  Range
 * fallback as above: an aggregate beyond 6e4 raises the flag and the pass is repeated on the fp32 path -- that batch's results are the
 * f32 mode's bytes.  pna_mfma=32 keeps the fp32 pipe, and with it f32-mode results.  The mode is the engine's: it survives
 * flowgnn_set_weights and new batches, and runs with embeddings, node embeddings, flowgnn_get_h, device batches, groups and option
 * hipgraph; sum and max pooling stay refused for PNA.  (DGN's f16 mode: flowgnn_set_model_numeric_mode, below.)
 */
/*
 * The numeric mode through the call that names the MODEL: model_id must be the engine's own model (FLOWGNN_ERR_ARG otherwise; the text
 * names both models; a null handle: FLOWGNN_ERR_ARG).  One call then reaches every mode any engine has:
 *   on a FLOWGNN_MODEL_DGN engine it accepts FLOWGNN_NUMERIC_F32, FLOWGNN_NUMERIC_Q6_10 (both as flowgnn_set_numeric_mode has them; Q6_10
 *   stays refused beside embeddings and the other outputs without a fixed-point form) and FLOWGNN_NUMERIC_F16: the one way to DGN's f16
 *   mode.  DGN's width is the reference's 100, so it has no width of its own to enter through as PNA has: flowgnn_set_numeric_mode,
 *   flowgnn_set_numeric_mode_dim and flowgnn_set_model_numeric_mode_dim(e, 100, FLOWGNN_NUMERIC_F16) keep returning
 *   FLOWGNN_ERR_UNSUPPORTED on a DGN engine, and the text names this call;
 *   on every other engine it IS flowgnn_set_model_numeric_mode_dim at that engine's own current width: FLOWGNN_EMB_DIM_PNA for PNA, the
 *   engine's width (flowgnn_set_emb_dim / flowgnn_set_model_emb_dim) for GIN and GCN, 100 for GIN-VN and GAT -- return code for return code.
 * FLOWGNN_NUMERIC_F16 for DGN changes the operands of the matrix-pipe products and nothing else.  Per layer:
 *   each feature of a source row h[u] is rounded to f16 ONCE, to nearest even (x_u; the default mode keeps a hi and a lo half);
 *   m1[v] = sum_{u->v} x_u is one MFMA per 32-source block, fp32 accumulation;
 *   the directional weight is d_uv = rne_f16((eig1[u] - eig1[v]) wscale_v) -- the fp32 subtraction and the exact power-of-two scale of
 *   the row first, then one rounding -- and pp[v] = sum x_u d_uv one MFMA per block; every further copy of a duplicate edge adds the
 *   same product x_u d_uv as its first;
 *   a1 = m1 / outdeg and a2 = |fma(-wsum wscale, h[v], pp) / (abssum wscale)| in fp32 as in the default mode, with h[v] unrounded;
 *   the dense update: a1 and a2 rounded to f16 once, to nearest even, the weights r(W s) (the hi halves of the default mode's split
 *   stream), ONE f16 x f16 MFMA per product in the default mode's accumulator order, the pre-scaled fp32 bias first;
 *   h' = h + relu(acc / s) in fp32.
 * fp32 and unchanged: the encoder, the row records (masks, wsum, abssum, out-degree), the residual, the rows and pooled rows that leave
 * the kernels, the mean pool and the 100 -> 50 -> 25 -> 1 head.  Range fallback as above: an a1, an a2 or -- in this mode -- any value of
 * h that is rounded as a source row beyond 6e4 raises the flag and the pass is repeated on the exact fp32 path: that batch's results are
 * the f32 mode's bytes (flowgnn_exact_reruns counts it).
 * The mode lives on the matrix-pipe kernels (the graph-resident kernel and the per-layer matrix-pipe kernel that flowgnn_get_h runs: their
 * taps are the mode's values, and the two agree in every byte on the same tiles, as in the default mode).  A job whose plan picks the
 * in-edge walk, the two-kernel layer or the fp32 pipe -- sparse jobs with E < 8 N, tiles under 0.4 fill, dgn_mfma=32, the exact re-run --
 * runs the default kernels and returns the f32 mode's bytes, as PNA's mode does under pna_mfma=32.  The mode is the engine's: it survives
 * flowgnn_set_weights and new batches, and runs with embeddings, node embeddings, flowgnn_get_h, device batches, groups and option
 * hipgraph (a recorded launch sequence is dropped on the switch); sum and max pooling stay refused for DGN.
 */
int flowgnn_set_model_numeric_mode(flowgnn_engine* e, int model_id, int mode);

/*
 * Pooling of the readout (GIN, GIN-VN, GCN, GAT): how a graph's last node rows r[v] (what
 * flowgnn_set_node_embeddings returns) become the vector the linear head is applied to.  v runs over every node of the graph --
 * GIN-VN's virtual node is a node, as it is for the mean.
 *   FLOWGNN_POOL_MEAN (default, the reference's finalize):  logit[g][t] = b[t] + W[t] . (sum_v r[v]) / n_g
 *   FLOWGNN_POOL_SUM  (the GIN paper's readout; OGB's graph_pooling = "sum"):  logit[g][t] = b[t] + W[t] . sum_v r[v]
 *   FLOWGNN_POOL_MAX  (graph_pooling = "max"):  logit[g][t] = b[t] + W[t] . m,  m[d] = max_v r[v][d]
 * The setting belongs to the engine, like the numeric mode: it may be changed between runs on a resident batch, it holds across
 * batches, and it drops a recorded launch sequence (option hipgraph).  In the default mode every launch is the one it always was.
 * Sum keeps the graph-resident kernels (instances whose readout leaves the division out) and the folded per-layer last stage; the
 * maximum is taken on chip for GIN and GIN-VN (the un-folded pooling instance) and from the rows of the per-layer path for GCN and
 * GAT, whose last stage is then un-folded (W . max is not a maximum of per-node scores).  A graph's sum has one order per path, as
 * the mean's has; no float atomics anywhere.  flowgnn_set_embeddings returns the vector the head is applied to, i.e. the sum or
 * the maximum under those modes; node embeddings and GAT's attention coefficients do not depend on the mode.  A NaN in a row does
 * not survive the maximum (v_max_f32 returns the other operand).
 * flowgnn_set_pooling: FLOWGNN_ERR_ARG for a mode outside 0..2.  FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why) for a mode
 *     other than the mean on PNA and DGN (their MLP heads were trained on the mean), in FLOWGNN_NUMERIC_Q6_10 (the fixed-point
 *     readout is the reference's), and while node logits are on (their contract is "the mean of the terms is the logit");
 *     flowgnn_set_numeric_mode and flowgnn_set_node_logits answer the same while a mode other than the mean is set.  Also while
 *     OGB's attention readout is on (flowgnn_set_attention_pooling, a readout of its own with a call of its own: there is no fourth mode).
 * flowgnn_pooling: the mode, -1 for a null handle.
 * flowgnn_group_set_pooling: flowgnn_set_pooling on every member.  flowgnn_entry_set_pooling: for the engines behind the
 *     <M>_compute_graphs entry points of `model`, as flowgnn_entry_set_option (remembered for engines created later).
 */
#define FLOWGNN_POOL_MEAN 0   /* default: the reference's */
#define FLOWGNN_POOL_SUM  1
#define FLOWGNN_POOL_MAX  2
int flowgnn_set_pooling(flowgnn_engine* e, int mode);
int flowgnn_pooling(const flowgnn_engine* e);            /* -1 for a null handle */

/*
 * Trained eps of GIN / GIN-VN.  OGB's GINConv computes mlp((1 + eps) x + propagate(...)) with eps an nn.Parameter; the reference
 * accelerator reads gin_ep1_eps_dim100.bin and never uses it, and so does this engine by default.  With eps on, layer l computes
 *     a[v] = s_l h_l[v] + sum_e relu(h_l[src_e] + ecomb_l[code_e]),     s_l = (float)(1.0f + eps[l]), formed once on the host
 * and everything behind `a` is what it was (operand split, range tracking on a, MLP, ReLU placement, readout).  GIN-VN's virtual node
 * is a node like any other.  In FLOWGNN_NUMERIC_F16 the product and the sum stay fp32, as the walk is; only the MLP operands are rounded.
 * "On" and "off" are states, not values: a non-null pointer turns the eps instances of the kernels on even if all five values are zero
 * (x * 1.0f == x: the same bits as off, through other kernels); NULL turns them off, and then every launch is the one it always was.
 * The setting belongs to the engine, like the pooling and the numeric mode: it holds across batches and across flowgnn_set_weights,
 * it may change between runs on a resident batch, and it drops a recorded launch sequence (option hipgraph).
 * flowgnn_load_weights_dir does not read the eps file; `host --eps` and the Python wrapper's load_weights_dir(dir, eps=True) do.
 * Kernels: single task, mean pooling, folded readout, no extra outputs -> gin_resident_eps_kernel (both front ends, both numeric
 * modes); every other configuration, the range fallback included -> the per-layer kernels' eps instances.
 * flowgnn_set_gin_eps: FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why) for any model but GIN / GIN-VN and in
 *     FLOWGNN_NUMERIC_Q6_10 (the fixed-point arithmetic is the reference's, which has no eps; flowgnn_set_numeric_mode(Q6_10) answers
 *     the same while eps is on); FLOWGNN_ERR_ARG for a value that is not finite.  While eps is on, flowgnn_run answers
 *     FLOWGNN_ERR_UNSUPPORTED under option gin_unfused 1, and so do flowgnn_run_aggregation_only and flowgnn_get_aggregate (the
 *     stand-alone aggregation kernel has no eps instance).
 * flowgnn_gin_eps: 1 on, 0 off, -1 for a null handle; eps_out (may be NULL) receives the five values (zeros while off).
 * "Five" is flowgnn_num_layers(e): after flowgnn_set_num_layers (below) both calls read and write that many floats.
 * flowgnn_group_set_gin_eps: flowgnn_set_gin_eps on every member.  flowgnn_entry_set_gin_eps: for the engines behind the
 *     GIN / GIN-VN entry points, one vector for every weight set.
 */
int flowgnn_set_gin_eps(flowgnn_engine* e, const float* eps /* [flowgnn_num_layers(e)] (5 unless flowgnn_set_num_layers said otherwise), NULL = off */);
int flowgnn_gin_eps(const flowgnn_engine* e, float* eps_out /* [flowgnn_num_layers(e)], may be NULL */);   /* 1 on, 0 off, -1 null handle */

/*
 * OGB's virtual node for GIN: the model of ogb/examples/graphproppred/mol with gnn_type = 'gin-virtual'.  It is NOT the reference's
 * GIN-VN (FLOWGNN_MODEL_GIN_VN), where the host appends an ordinary node joined to every atom: OGB keeps one vector per graph beside
 * the nodes and updates it with a small MLP between layers.  With D = 100, five GIN layers, and the BatchNorms of the virtual-node MLP
 * folded into its linear layers (both sit in front of a ReLU, so folding is exact; flowgnn_amd/export.py does it):
 *     vn_0[g] = vn_embedding                                                      for every graph g
 *     for l = 0 .. 4:
 *         x_l[v]  = h_l[v] + vn_l[g(v)]                                           (fp32, one rounding; the last layer too)
 *         h_{l+1} = GIN layer l applied to x_l                                    (messages, self term with eps if on, MLP, ReLU as ever)
 *         if l < 4:  t = sum over v in g of x_l[v] + vn_l[g]                      (always a sum, whatever flowgnn_set_pooling says)
 *                    vn_{l+1}[g] = relu(w2[l] relu(w1[l] t + b1[l]) + b2[l])
 *     readout: unchanged, on h_5
 * Tensors (host arrays, copied by the call): vn_embedding [100], w1 [4][200][100], b1 [4][200], w2 [4][100][200], b2 [4][100].
 * All five NULL turns it off (the default), and then every launch is the one it always was; some but not all NULL, or a value that
 * is not finite, is FLOWGNN_ERR_ARG.  The setting belongs to the engine, like eps: it holds across batches and flowgnn_set_weights,
 * it may change between runs on a resident batch, and it drops a recorded launch sequence (option hipgraph).  It combines with eps
 * (OGB's gin-virtual has both), with every pooling mode, NUM_TASK, the optional outputs, device batches and groups.  In
 * FLOWGNN_NUMERIC_F16 only the node MLP's operands are rounded, as ever; the virtual node's arithmetic is fp32 FMAs.
 * Kernels: one launch per layer (profile slot gin_ogb_vn) in front of the per-layer kernels, which every batch takes while it is on
 * -- the graph-resident kernels do not carry the vector.  A graph's logit has the same bits wherever the
 * graph stands in a batch, a slice or a group's cut.  flowgnn_get_h returns h_5 as ever; the rows the layers leave in HBM on the way
 * are x_l (after the add), not h_l.
 * FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why): any model but FLOWGNN_MODEL_GIN (GCN has flowgnn_set_gcn_virtual_node below); FLOWGNN_NUMERIC_Q6_10, in both orders of
 * the two setters; and, while it is on, flowgnn_run_aggregation_only and flowgnn_get_aggregate.
 * flowgnn_ogb_virtual_node: 1 on, 0 off, -1 for a null handle.  flowgnn_group_set_ogb_virtual_node: the setter on every member.
 * The reference has no such model, so the reference-compatible <M>_compute_graphs entry points have no form of it.
 * Files: gin_ep1_virtualnode_dim100.bin beside the GIN set holds the five tensors in this order (161 300 LE float32);
 * flowgnn_load_weights_dir does not read it; `host GIN --ogb-vn` and the Python wrapper's load_weights_dir(dir, virtual_node=True) do.
 */
#define FLOWGNN_OGB_VN_LAYERS 4
#define FLOWGNN_OGB_VN_HIDDEN 200
int flowgnn_set_ogb_virtual_node(flowgnn_engine* e, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2); /* host arrays, copied; all NULL = off */
int flowgnn_ogb_virtual_node(const flowgnn_engine* e);            /* 1 on, 0 off, -1 null handle */

/*
 * The same model through a call that carries the tensors' width, which is how OGB's gin-virtual at its default emb_dim 300 runs
 * (flowgnn_set_emb_dim(e, FLOWGNN_EMB_DIM_OGB) first).  With D = emb_dim: vn_embedding [D], w1 [4][2D][D], b1 [4][2D], w2 [4][D][2D],
 * b2 [4][D]; the definition is the one above with that D.  The leading 4 is flowgnn_num_layers(e) - 1: after flowgnn_set_num_layers
 * (below) the call reads that many updates, and the definition's "l = 0 .. 4" and "l < 4" run over the engine's depth.
 *   emb_dim == 100: exactly flowgnn_set_ogb_virtual_node -- the same state, the same kernels, the same bits.
 *   emb_dim == 300: kernels of gin_wide.hip.  No launch rewrites the rows to add a vector: x_0 = h_0 + E is
 *       formed in the atom encoder, x_{l+1} in the epilogue of layer l's kernel, t by one read of the rows (profile slot
 *       gin_wide_vn_pool) and the update MLP by the layer kernel's own split-f16 products on G rows (gin_wide_vn_update), with the
 *       fp32 re-run of flowgnn_exact_reruns when t or a hidden value leaves the f16 range.  It combines with eps, NUM_TASK, every
 *       pooling mode, the optional outputs, flowgnn_get_h, device batches and groups; the bits of a graph's result do not depend on
 *       where the graph stands in a batch.
 * FLOWGNN_ERR_ARG: emb_dim other than 100 or 300; tensors given and emb_dim != flowgnn_emb_dim(e) (flowgnn_last_error names both);
 * some of the five NULL and some not; a value that is not finite.  FLOWGNN_ERR_UNSUPPORTED: any model but FLOWGNN_MODEL_GIN.  All five
 * NULL turns the virtual node off at any width.  flowgnn_set_ogb_virtual_node itself has no width argument, so its tensors are 100
 * wide by contract and it keeps refusing at width 300.  flowgnn_ogb_virtual_node reports 1 for either width.  While a virtual node of
 * either width is on, flowgnn_set_emb_dim to the other width is FLOWGNN_ERR_UNSUPPORTED: the tensors belong to a width -- turn it off,
 * change the width, set it again.  State handling is that of the call above.
 * Files: gin_ep1_virtualnode_dim300.bin holds the five tensors in this order (1 443 900 LE float32); `host GIN --emb-dim 300 --ogb-vn`
 * and the Python wrapper's load_weights_dir(dir, virtual_node=True) read the file of the engine's width.
 */
int flowgnn_set_ogb_virtual_node_dim(flowgnn_engine* e, int emb_dim, const float* vn_embedding, const float* w1, const float* b1,
                                     const float* w2, const float* b2); /* host arrays, copied; all NULL = off */

/*
 * OGB's virtual node for GCN: gnn_type = 'gcn-virtual' of the same example.  The five tensors, their shapes, the folding and the
 * device form are those of flowgnn_set_ogb_virtual_node above; the definition differs where GCN does -- the layer's linear map comes
 * first, so the vector passes through it:
 *     vn_0[g] = vn_embedding
 *     for l = 0 .. 4:
 *         x_l[v]  = h_l[v] + vn_l[g(v)]                                           (the last layer too; h_0 = the atom encoder's rows)
 *         h_{l+1} = GCN layer l applied to x_l                                    (W_l x_l + b_l FIRST, then messages, root term, BatchNorm, ReLU
 *                                                                                  but after layer 4 -- all as ever)
 *         if l < 4:  t = sum over v in g of x_l[v] + vn_l[g]                      (always a sum, whatever flowgnn_set_pooling says)
 *                    vn_{l+1}[g] = relu(w2[l] relu(w1[l] t + b1[l]) + b2[l])
 *     readout: unchanged
 * Calls of its own, because flowgnn_set_ogb_virtual_node on a GCN engine is refused and stays so.  All five NULL turns it off (the
 * default), and then every launch is the one it always was; some but not all NULL, a value that is not finite, or a null handle is
 * FLOWGNN_ERR_ARG.  The setting holds across batches and flowgnn_set_weights, may change between runs on a resident batch, and drops
 * a recorded launch sequence (option hipgraph).  It combines with every pooling mode, NUM_TASK, the optional outputs, device batches
 * and groups.  flowgnn_get_h returns x_4 as ever, now with vn_4 inside.
 * Kernels: while it is on every batch takes the per-layer kernels.  In the default configuration the add and
 * the per-graph sums happen in the registers of the fused layer kernels and one small launch per update (profile slot gcn_ogb_vn,
 * four per run) forms vn_{l+1}; the sums are cut at the batch's 16-node tiles, so a graph's logit has the same bits from run to run
 * and between a host batch and the same batch given on the device, and agrees within fp32 rounding when the graph stands elsewhere
 * (a permuted batch, a slice, a group's cut).  The configurations that do not fuse (gcn_mfma 32, gcn_unfused 1, the exact re-run
 * behind the range flag, a batch without edges) add the vector in place in front of each dense launch (profile slot gin_ogb_vn, five
 * per run), with GIN's bit invariance.
 * FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why): any model but FLOWGNN_MODEL_GCN; FLOWGNN_NUMERIC_Q6_10, in both orders of
 * the two setters; and, while it is on, flowgnn_run_aggregation_only and flowgnn_get_aggregate.
 * flowgnn_gcn_virtual_node: 1 on, 0 off, -1 for a null handle.  flowgnn_group_set_gcn_virtual_node: the setter on every member.
 * GCN_compute_graphs has no form of it.
 * Files: gcn_ep1_virtualnode_dim100.bin beside the GCN file holds the five tensors in this order (161 300 LE float32);
 * flowgnn_load_weights_dir does not read it; `host GCN --ogb-vn` and the Python wrapper's load_weights_dir(dir, virtual_node=True) do.
 */
int flowgnn_set_gcn_virtual_node(flowgnn_engine* e, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2); /* host arrays, copied; all NULL = off */
int flowgnn_gcn_virtual_node(const flowgnn_engine* e);            /* 1 on, 0 off, -1 null handle */

/*
 * gcn-virtual through a call that carries the tensors' width, which is how it runs at OGB's default emb_dim 300
 * (flowgnn_set_model_emb_dim(e, FLOWGNN_EMB_DIM_OGB) first): the mirror of flowgnn_set_ogb_virtual_node_dim.  With D = emb_dim:
 * vn_embedding [D], w1 [4][2D][D], b1 [4][2D], w2 [4][D][2D], b2 [4][D]; the definition is the one above with that D.  The leading 4 is
 * flowgnn_num_layers(e) - 1, as in flowgnn_set_ogb_virtual_node_dim.
 *   emb_dim == 100: exactly flowgnn_set_gcn_virtual_node -- the same state, the same kernels, the same bits.
 *   emb_dim == 300: kernels of gcn_wide.hip.  The row the vector is added to exists only in the registers
 *       of the fused layer kernel, so its VN instance adds vn there, in front of the f16 split, and leaves the per-graph sums as
 *       partial rows cut at the batch's 16-node tiles (section 4.15's scheme); vn_0 = E sits in layer 0's bias.  Profile slots:
 *       gcn_wide_vn_t0 (sum of the atom rows, once), gcn_wide_vn_t (three) and gcn_wide_vn_update (four, gin_wide.hip's split-f16
 *       update MLP), with the fp32 re-run of flowgnn_exact_reruns when a row, t or a hidden value leaves the f16 range.  It combines
 *       with NUM_TASK, every pooling mode, the optional outputs, flowgnn_get_h, device batches and groups.  A graph's result has the
 *       same bits from run to run and between a host batch and the same batch given on the device, and agrees within fp32 rounding
 *       when the graph stands elsewhere (a permuted batch, a slice, a group's cut).
 * FLOWGNN_ERR_ARG: emb_dim other than 100 or 300; tensors given and emb_dim != flowgnn_emb_dim(e) (flowgnn_last_error names both);
 * some of the five NULL and some not; a value that is not finite; a null handle.  FLOWGNN_ERR_UNSUPPORTED: any model but
 * FLOWGNN_MODEL_GCN; FLOWGNN_NUMERIC_Q6_10.  All five NULL turns the virtual node off at any width.  flowgnn_set_gcn_virtual_node
 * itself has no width argument, so its tensors are 100 wide by contract and it keeps refusing at width 300.
 * flowgnn_gcn_virtual_node reports 1 for either width.  While a virtual node of either width is on, flowgnn_set_model_emb_dim to the
 * other width is FLOWGNN_ERR_UNSUPPORTED: turn it off, change the width, set it again.  State handling is that of the call above.
 * Files: gcn_ep1_virtualnode_dim300.bin holds the five tensors in this order (1 443 900 LE float32); `host GCN --emb-dim 300 --ogb-vn`
 * and the Python wrapper's load_weights_dir(dir, virtual_node=True) read the file of the engine's width.
 */
int flowgnn_set_gcn_virtual_node_dim(flowgnn_engine* e, int emb_dim, const float* vn_embedding, const float* w1, const float* b1,
                                     const float* w2, const float* b2); /* host arrays, copied; all NULL = off */

/*
 * OGB's graph_pooling="attention" readout for GIN and GCN at width 300, with or without OGB's virtual node:
 *     GlobalAttention(gate_nn = Sequential(Linear(D, 2D), BatchNorm1d(2D), ReLU(), Linear(2D, 1)))
 * With D = emb_dim = 300, H = 2D and r[v] the rows the readout pools (h_5 of GIN, GCN's final rows: exactly what
 * flowgnn_set_node_embeddings returns):
 *     s[v]        = w2 . relu(W1 r[v] + b1)                  W1 [H][D], b1 [H], w2 [H]; the BatchNorm folded into W1, b1 by the exporter
 *     m_g         = max over v in g of s[v]
 *     e[v]        = exp(s[v] - m_g)
 *     pooled[g]   = (sum over v in g of e[v] r[v]) / (sum over v in g of e[v])     both sums in node order, one chain per column
 *     logit[g][t] = b[t] + W[t] . pooled[g]                  the model's own head, every NUM_TASK
 * The bias of the gate's last Linear (OGB's pool.gate_nn.3.bias) cancels in the softmax: it is neither taken nor stored.  A one-node
 * graph gets pooled = r[v] exactly (e = 1, Z = 1), so its logit has the bits of the mean readout's.  A graph without nodes gets zeros.
 * Arithmetic: the first product is fp32-accurate on the f16 matrix pipe (three split-f16 MFMAs, W1 pre-scaled by a power of two and
 * split on the host), with the fp32 re-run of flowgnn_exact_reruns when a row or a hidden value leaves the f16 range; everything else
 * is fp32.  The bits of a graph's result depend on that graph alone (profile slots attn_gate, attn_pool_rows).
 * The tensors are host arrays and are copied.  All three NULL turns the readout off (the default) at any width and for any model, and
 * then every launch is the one it always was.  The setting holds across batches and flowgnn_set_weights, may change between runs on a
 * resident batch, and drops a recorded launch sequence (option hipgraph).  It combines with eps, NUM_TASK, OGB's virtual node, graph
 * embeddings (they return pooled), node embeddings, flowgnn_get_h, host and device batches, groups and option hipgraph.
 * FLOWGNN_ERR_ARG: a null handle; emb_dim other than 100 or 300; some of the three NULL and some not; a value that is not finite;
 * tensors given and emb_dim != flowgnn_emb_dim(e) (flowgnn_last_error names both widths).
 * FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why): any model but FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN; emb_dim == 100 (only
 * the 300-wide models have this readout: flowgnn_set_emb_dim / flowgnn_set_model_emb_dim first); in both orders of the two calls,
 * flowgnn_set_pooling other than the mean (while the readout is on the mean is the only accepted value, and flowgnn_pooling keeps
 * reporting what flowgnn_set_pooling said) and flowgnn_set_node_logits (the logit is no longer a mean of per-node terms); and, while it
 * is on, a change of width: the tensors belong to a width -- turn it off, change the width, set it again.
 * flowgnn_attention_pooling: 1 on, 0 off, -1 for a null handle.  flowgnn_group_set_attention_pooling: the setter on every member.
 * The <M>_compute_graphs entry points have no form of it, as they have none at width 300.
 * Files: gin_ep1_attnpool_dim300.bin / gcn_ep1_attnpool_dim300.bin beside the model's set hold w1, b1, w2 in this order (181 200 LE
 * float32); flowgnn_load_weights_dir does not read it; `host GIN|GCN --emb-dim 300 --attn-pool` and the Python wrapper's
 * load_weights_dir(dir, attention_pooling=True) do.
 */
int flowgnn_set_attention_pooling(flowgnn_engine* e, int emb_dim, const float* w1, const float* b1, const float* w2); /* host arrays, copied; all NULL = off */
int flowgnn_attention_pooling(const flowgnn_engine* e);   /* 1 on, 0 off, -1 null handle */

/*
 * OGB's graph_pooling="set2set" readout for GIN and GCN at width 300 (gin, gin-virtual, gcn, gcn-virtual): OGB pools with PyG's
 * Set2Set(emb_dim, processing_steps) -- an LSTM(2D, D) over the graphs' query vectors -- and reads a head of its own, Linear(2D, NUM_TASK).
 * With D = emb_dim = 300, r[v] the rows the readout pools (exactly what flowgnn_set_node_embeddings returns) and g(v) the graph of v:
 *     h_0 = c_0 = 0 [G][D];  q*_0 = 0 [G][2D]
 *     for t = 1 .. steps:
 *         z      = W_ih q*_{t-1} + b_ih + W_hh h_{t-1} + b_hh        [G][4D] = (z_i, z_f, z_g, z_o): torch.nn.LSTM's gate order
 *         c_t    = sigmoid(z_f) c_{t-1} + sigmoid(z_i) tanh(z_g)
 *         h_t    = sigmoid(z_o) tanh(c_t)
 *         e[v]   = r[v] . h_t[g(v)]
 *         m_g    = max over v in g of e[v];  a[v] = exp(e[v] - m_g)
 *         r_t[g] = (sum over v in g of a[v] r[v]) / (sum over v in g of a[v])    both sums in node order, one chain per column
 *         q*_t   = [h_t, r_t]
 *     logit[g][k] = head_b[k] + head_w[k] . q*_steps[g]
 * w_ih [4D][2D], w_hh [4D][D], b_ih [4D], b_hh [4D] are PyG's pool.lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0; head_w
 * [num_tasks][2D] and head_b [num_tasks] are OGB's graph_pred_linear.  While the readout is on the model's own [NUM_TASK][D] head is not
 * read.  A graph without nodes has r_t = 0 and still gets a logit from h_t; a one-node graph has r_t = r[v] exactly.  q*'s first half
 * is h_{t-1}, so the engine folds w_hh into w_ih's first D columns and the two biases into one, in float64, rounded once; at t = 1 the
 * product is skipped (z is the bias).  Arithmetic: the product is fp32-accurate on the f16 matrix pipe (three split-f16 MFMAs, the
 * weights pre-scaled by a power of two and split on the host), with the fp32 re-run of flowgnn_exact_reruns when a value of q* leaves
 * the f16 range; the cell, the dots, the softmax and the head are fp32, the cell safe at saturation.  Every sum has a fixed order, there
 * are no atomics, and the bits of a graph's logit depend on that graph alone (profile slots s2s_lstm,
 * s2s_dot_rows, s2s_pool_rows, s2s_head).
 * The tensors are host arrays and are copied.  All six NULL turns the readout off (the default) at any width and for any model, and
 * then every launch is the one it always was.  The setting holds across batches and flowgnn_set_weights, may change between runs on a
 * resident batch, and drops a recorded launch sequence (option hipgraph).  It combines with eps, NUM_TASK, OGB's virtual node, GIN's f16
 * numeric mode at width 300 (the readout stays fp32-accurate), node embeddings, flowgnn_get_h, host and device batches, groups and
 * option hipgraph.
 * FLOWGNN_ERR_ARG: a null handle; emb_dim other than 100 or 300; some of the six NULL and some not; and, with tensors given: steps
 * outside 1 .. FLOWGNN_SET2SET_MAX_STEPS; num_tasks < 1 or != flowgnn_num_tasks(e) (flowgnn_last_error names both numbers); a value
 * that is not finite; emb_dim != flowgnn_emb_dim(e) (flowgnn_last_error names both widths).
 * FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why): any model but FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN; emb_dim == 100; in
 * both orders of the two calls, flowgnn_set_pooling other than the mean, flowgnn_set_node_logits, flowgnn_set_attention_pooling (the
 * two readouts exclude each other) and flowgnn_set_embeddings (the vector the head reads is 2D wide and every embeddings buffer is D
 * wide); and, while it is on, a change of width and a change of NUM_TASK: turn it off, change, set it again.
 * flowgnn_set2set_pooling: the steps when on, 0 off, -1 for a null handle.  flowgnn_group_set_set2set_pooling: the setter on every
 * member.  The <M>_compute_graphs entry points have no form of it.
 * Files: gin_ep1_set2set_dim300.bin / gcn_ep1_set2set_dim300.bin beside the model's set hold w_ih, w_hh, b_ih, b_hh, head_w, head_b in
 * this order as LE float32 (NUM_TASK follows from the length); flowgnn_load_weights_dir does not read it; `host GIN|GCN --emb-dim 300
 * --set2set [--set2set-steps N]` and the Python wrapper's load_weights_dir(dir, set2set=True, set2set_steps=N) do.
 */
#define FLOWGNN_SET2SET_MAX_STEPS 8
int flowgnn_set_set2set_pooling(flowgnn_engine* e, int emb_dim, int steps, int num_tasks, const float* w_ih, const float* w_hh,
                                const float* b_ih, const float* b_hh, const float* head_w, const float* head_b); /* host arrays, copied; all six NULL = off */
int flowgnn_set2set_pooling(const flowgnn_engine* e);   /* steps when on, 0 off, -1 null handle */

/*
 * OGB's JK="sum" and residual=True for GIN at width 300 (gin and gin-virtual): the two arguments of OGB's
 * GNN(...) that change the forward pass without adding a parameter.  A state_dict of such a model goes through the exporter
 * unchanged, so the CALLER passes the flags; without this call a checkpoint trained with either runs as JK="last", residual=False.
 * In the notation of flowgnn_set_ogb_virtual_node_dim (y_l: GIN layer l of its input rows x_l, ReLU'd for l < 4; x_l = h_l without
 * the virtual node), every add fp32 in every numeric mode:
 *     h_{l+1}[v] = y_l[v] + x_l[v]                     residual: one add after the ReLU, the last layer included
 *     x_{l+1}[v] = h_{l+1}[v] + vn_{l+1}[g(v)]         virtual node, l < 4: after the residual's add
 *     vn_{l+1}[g] = vn_l[g] + relu(w2 relu(w1 t + b1) + b2)      residual with the virtual node (vn_0 = E)
 *     r[v] = ((((x_0[v] + x_1[v]) + x_2[v]) + x_3[v]) + x_4[v]) + h_5[v]      JK sum: six terms, left to right
 * so the residual and the JK sum see the rows with the virtual node's vector inside, as OGB's GNN_node_Virtualnode has them.  The six
 * terms are those of OGB's current source (range(num_layer + 1)); older releases summed range(num_layer), five terms.
 * r is what the readout pools (every pooling, the attention and set2set readouts, every NUM_TASK), what node embeddings return (their
 * contract is "the rows the pool is taken over") and what node logits are computed from.  flowgnn_get_h keeps returning the last
 * layer's output h_5 (with the residual when it is on): under JK sum that is NOT what the readout pools.
 * The setting is the engine's, like the pooling mode: it holds across batches and flowgnn_set_weights, may change between runs on a
 * resident batch, and drops a recorded launch sequence (option hipgraph).  (FLOWGNN_JK_LAST, 0) is the default: every launch is the one
 * it always was, setting it is the same as never calling, and it is accepted wherever the handle is valid.  It combines with a trained
 * eps, the virtual node, FLOWGNN_NUMERIC_F16 at width 300 and its exact re-run, host and device batches and groups.
 * FLOWGNN_ERR_ARG: a null handle; jk outside 0..1; residual outside 0..1; emb_dim other than 100 or 300; a non-default setting with
 * emb_dim != flowgnn_emb_dim(e) (flowgnn_last_error names both widths).
 * FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why), for a non-default setting: any model but FLOWGNN_MODEL_GIN (GCN's rows in HBM
 * are post-linear: that form does not exist yet under this call -- it is flowgnn_set_model_jk_residual, below, that carries it);
 * width 100 (the graph-resident kernels and the 100-wide per-layer path have no instance); and, while it is on, flowgnn_set_emb_dim /
 * flowgnn_set_model_emb_dim to 100: turn it off, then change the width.
 * flowgnn_jk_residual: 1 if either is on, 0 off, -1 for a null handle; the outs may be NULL.  flowgnn_group_set_jk_residual: the setter
 * on every member.  The <M>_compute_graphs entry points have no form of it.  `host GIN --emb-dim 300 --jk sum --residual`.
 */
#define FLOWGNN_JK_LAST 0
#define FLOWGNN_JK_SUM  1
int flowgnn_set_jk_residual(flowgnn_engine* e, int emb_dim, int jk, int residual);   /* (LAST, 0) = off, the default */
int flowgnn_jk_residual(const flowgnn_engine* e, int* jk_out, int* residual_out);    /* 1 if either is on, 0 off, -1 null handle; outs may be NULL */

/*
 * The same two options for GCN at width 300 (OGB's gcn and gcn-virtual), through a call that carries the model
 * as flowgnn_set_model_emb_dim does beside flowgnn_set_emb_dim: flowgnn_set_jk_residual keeps refusing FLOWGNN_MODEL_GCN.  On a GIN
 * engine this call IS that one (same state, same codes); flowgnn_jk_residual serves both.  conv.py's GNN_node / GNN_node_Virtualnode
 * with gnn_type="gcn", in the notation above with conv_l GCN layer l (the product W_l x + b_l, the walk, root, 1 / (deg + 1) and the
 * folded BatchNorm) and y_l = relu(conv_l(x_l)) for l < 4, y_4 = conv_4(x_4):
 *     x_0[v] = h_0[v] (+ E)                            h_0: the UNPROJECTED atom-encoder rows
 *     h_{l+1}[v] = y_l[v] + x_l[v]                     residual: one fp32 add after the ReLU, the last layer included
 *     x_{l+1}[v] = h_{l+1}[v] + vn_{l+1}[g(v)]         virtual node, l < 4: one fp32 add after the residual's
 *     vn_{l+1}[g] = vn_l[g] + relu(w2 relu(w1 t + b1) + b2),  t = sum_{v in g} x_l[v] + vn_l[g]     (vn_0 = E)
 *     r[v] = ((((x_0[v] + x_1[v]) + x_2[v]) + x_3[v]) + x_4[v]) + h_5[v]      JK sum: six terms, left to right
 * r, flowgnn_get_h (h_5, with the residual when it is on), the state and the default are as above.  It combines with
 * flowgnn_set_gcn_virtual_node_dim, the three poolings, the attention and set2set readouts, NUM_TASK, every optional output, host and
 * device batches, groups, option hipgraph and the exact re-run.
 * FLOWGNN_ERR_ARG: as above.  FLOWGNN_ERR_UNSUPPORTED for a non-default setting: any model but FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN;
 * GCN at width 100 (flowgnn_set_model_emb_dim(e, 300) first); and, while it is on, flowgnn_set_model_emb_dim to 100.
 * flowgnn_group_set_model_jk_residual: on every member.  `host GCN --emb-dim 300 [--ogb-vn] --jk sum --residual`.
 */
int flowgnn_set_model_jk_residual(flowgnn_engine* e, int emb_dim, int jk, int residual);   /* (LAST, 0) = off, the default */

/*
 * OGB's num_layer for GIN and GCN at width 300 (gin, gin-virtual, gcn, gcn-virtual): the depth of the model as
 * a run-time property of the engine, 5 by default as in the reference (a compile-time constant there).  The 300-wide paths launch one
 * kernel per layer, so the depth is the bound of a host-side loop: the layer kernels are the ones every depth-5 run launches, L times.
 * With L = num_layers every "5" of the tensors above is L and every "4" of the virtual node's is L - 1:
 *     GIN  edge_emb [L][13][300], w1 [L][600][300], b1 [L][600], w2 [L][300][600], b2 [L][300]
 *     GCN  edge_emb [L][13][300], convs_weight [L][300][300], convs_bias / root_emb / bn_* [L][300]
 *     flowgnn_set_gin_eps reads and flowgnn_gin_eps writes L floats; the virtual-node setters read L - 1 updates
 *     JK sum has L + 1 terms; flowgnn_get_h returns h_L, the last layer's output
 * flowgnn_load_weights_dir reads the same file names, sized by L, and refuses a file whose size is that of another depth (the text
 * names both depths) instead of reading short or past its end.
 * The range is FLOWGNN_MIN_NUM_LAYERS .. FLOWGNN_MAX_NUM_LAYERS: OGB's GNN_node raises below 2, and 8 is the size of the arrays this
 * ABI keeps per layer (eps, the self scales).
 * A change follows flowgnn_set_num_tasks: the model drops its weights, the batch has to be set again, a recorded launch sequence is
 * dropped.  The numeric mode, the pooling, the attention / set2set readouts and JK / residual survive it: none is sized by the depth.
 * The depth the engine has is a no-op (FLOWGNN_OK before any state changes), so flowgnn_set_num_layers(e, w, 5) on an engine that
 * never called it changes nothing, at either width.
 * FLOWGNN_ERR_ARG: a null handle; num_layers outside 2 .. 8; emb_dim other than 100 or 300; emb_dim != flowgnn_emb_dim(e)
 * (flowgnn_last_error names both widths).
 * FLOWGNN_ERR_UNSUPPORTED (flowgnn_last_error says why): any model but FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN; width 100 with a depth
 * other than 5 (the graph-resident and the 100-wide per-layer kernels are five layers deep); while a trained eps or OGB's virtual node
 * is on (their tensors belong to a depth: turn it off, change the depth, set it again); FLOWGNN_NUMERIC_Q6_10; and, while the depth is
 * not 5, flowgnn_set_emb_dim / flowgnn_set_model_emb_dim to 100 (set the depth back to 5 first).
 * flowgnn_num_layers: the engine's depth, 5 on every engine that never called the setter, -1 for a null handle.
 * flowgnn_group_set_num_layers: the setter on every member.  The <M>_compute_graphs entry points have no form of it.
 * `host GIN|GCN --emb-dim 300 --num-layer N`.
 */
#define FLOWGNN_NUM_LAYERS_DEFAULT 5
#define FLOWGNN_MIN_NUM_LAYERS 2
#define FLOWGNN_MAX_NUM_LAYERS 8
int flowgnn_set_num_layers(flowgnn_engine* e, int emb_dim, int num_layers);   /* GIN, GCN at width 300: 2 .. 8; 5 = the default */
int flowgnn_num_layers(const flowgnn_engine* e);                              /* -1 for a null handle */

/*
 * Laplacian eigenvectors: DGN's node_eigen from the graphs alone (the reference reads it from DGN/eig/g%d.txt and does not say where it
 * comes from).  For graph g with n nodes and edges (u, v) in local ids:
 *     A[u][v] = A[v][u] = 1 for every edge with u != v   (both directions and duplicates collapse to 1, self loops are ignored)
 *     d[i] = max(1, sum_j A[i][j]),   L = I - D^-1/2 A D^-1/2          (an isolated node has L[i][i] = 1)
 *     node_eigen[noff[g] + i][k] = v_k[i] for k < min(4, n), 0 for k >= n,   (lambda_k, v_k) the eigenpairs of L, lambda ascending,
 * every v_k of unit 2-norm -- what the upstream DGN preprocessing computes for a graph that lists both directions of its edges.  The
 * sign of a vector is whatever the rotations leave (DGN sees neither the sign nor the scale of column 1); inside a repeated
 * eigenvalue the basis is arbitrary but orthonormal.  fp32: a cyclic Jacobi iteration in on-chip memory, one workgroup per graph
 * (DESIGN.md section 4.13); residual |L v - lambda v| <= 8 max(n, 8) 2^-24.  A graph's vectors depend on that graph alone: they are
 * bit-identical whatever the batch order, the slice, the other graphs of the call, or which of the two functions computes them.
 *  Any model's engine will do: only its device and its launch stream are used.  Neither function touches the resident batch, a
 *  recorded launch sequence (option hipgraph) or any output.  FLOWGNN_ERR_ARG for nulls and bad counts, as flowgnn_set_batch gives;
 *  FLOWGNN_ERR_UNSUPPORTED, with a flowgnn_last_error text naming the first such graph, for a graph of more than
 *  FLOWGNN_EIGEN_MAX_NODES nodes -- nothing is launched or written then.  num_graphs == 0: FLOWGNN_OK, nothing is launched.
 *  flowgnn_laplacian_eigen_max_nodes: 128.  Needs no GPU.
 *  flowgnn_laplacian_eigen: host arrays, synchronous (upload, run, copy back); FLOWGNN_ERR_EDGE_RANGE for an endpoint outside [0, n).
 *  flowgnn_laplacian_eigen_device: flowgnn_set_batch_device's contract -- host counts, DEVICE edge_list in either layout
 *     (FLOWGNN_LAYOUT_REFERENCE: int32 [E][2], local ids; FLOWGNN_LAYOUT_PYG: int64 [2][E], batch-global ids, made local as
 *     id - noff[g]) and DEVICE node_eigen (float32 [N][4]), both checked as that function checks its arrays; asynchronous on the
 *     engine's launch stream, so a following flowgnn_set_batch_device that reads node_eigen needs no event; an edge with an endpoint
 *     outside its graph is skipped (flowgnn_set_batch_device refuses such a batch afterwards anyway).  Offsets and size-class lists
 *     live in engine-owned scratch that only grows: no allocation per call in the steady state.
 */
#define FLOWGNN_EIGEN_MAX_NODES 128
int flowgnn_laplacian_eigen_max_nodes(void);
int flowgnn_laplacian_eigen(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                            const int* edge_list /* host [E][2], local ids */, float* node_eigen /* host [N][4] */);
int flowgnn_laplacian_eigen_device(flowgnn_engine* e, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                                   int layout, const void* edge_list /* device */, float* node_eigen /* device [N][4] */);

/*
 * Run-time switches, by name (the full list with defaults: the option table in flowgnn_amd/csrc/engine.hip, or
 * flowgnn_option_count / flowgnn_option_name).  They select between kernels that compute the SAME results -- e.g.
 * "gin_resident" 0 = one launch per layer, "gin_mfma" 32 = fp32 matrix pipe instead of three f16 products, "pna_fused" 0 =
 * separate aggregation and dense kernels, "hipgraph" 1 -- and exist for A/B measurements and parity tests.  Defaults come from the
 * table; the environment is read in exactly one place, when flowgnn_create builds an engine (FLOWGNN_<KEY IN UPPER CASE>, "f32"
 * reads as 32), and flowgnn_set_option overrides it.  Call it before flowgnn_set_batch: it invalidates the resident batch.
 * Unknown key: FLOWGNN_ERR_UNSUPPORTED.  No option changes the shape of any buffer.  ONE shipped option changes results, by
 * design: "gat_reference_quirk" (1 = read the node features without the per-graph offset, as GAT/src/GAT_compute.cc:72
 * does; 0, the default = with it); every other one selects between kernels that agree to
 * fp32 rounding (bit for bit where DESIGN.md says so).  The kernels' ablation hooks -- which do give wrong results, for per-phase
 * timing -- are compiled in only with -DFLOWGNN_DEV.  "gin_pingpong" != 0 implies the three-kernel front end ("gin_tile_build" 0).
 */
int flowgnn_set_option(flowgnn_engine* e, const char* key, double value);
int flowgnn_get_option(const flowgnn_engine* e, const char* key, double* value);
int flowgnn_option_count(void);
const char* flowgnn_option_name(int i);

/*
 * Several devices behind one handle (north_star: the batch dimension partitioned across the GPUs of a node; the reference has
 * one compute unit, GIN/config_slr.cfg:1-2).  One engine + one host thread per listed device; flowgnn_group_set_batch cuts the
 * batch into contiguous graph ranges balanced by sum(N + E) (flowgnn_shard_ranges: cuts[0..parts], cuts[r] = the first graph
 * whose cumulative node + edge count reaches r / parts of the total) and flowgnn_group_get_results writes [num_graphs][NUM_TASK]
 * in job order.  A device may appear more than once in the list.  flowgnn_group_engine(g, i) exposes member i for per-engine
 * calls (profiling, taps; a flowgnn_set_batch on a member makes flowgnn_group_run / get_results refuse until the next
 * flowgnn_group_set_batch).  Every engine has a persistent host thread: a group call costs microseconds of host time.
 * What a group's results are relative to ONE engine holding the whole job: graphs are independent and every kernel sums a row's
 * in-edges in an order that depends on the row alone, so results are BIT-IDENTICAL whenever the same kernels run -- and the
 * kernels are chosen from the JOB's totals, which the group (and the entry points' ranges) hand down to every member through
 * flowgnn_set_job_totals.  That covers GIN, GIN-VN, GCN, GAT and PNA with default options at any device count.  Two exceptions:
 * DGN's matrix-pipe aggregation (default on kNN-dense jobs, option "dgn_mfma_agg") sums in tile order -- equal to 1e-5 relative
 * under a different cut, bit-identical with "dgn_mfma_agg" 0; and a multi-PROCESS caller
 * that cuts a job of LARGE graphs whose tiles are about as full as the resident kernels' fill threshold must hand the job's fill down
 * itself (flowgnn_graph_tile_fill + flowgnn_set_job_tile_fill, as the group does), or a shard can pack to the other side of the
 * threshold and run the per-layer kernels: fp32 rounding differences.  flowgnn_group_run / get_results / shards answer FLOWGNN_ERR_STATE unless the engines hold
 * the shards of a flowgnn_group_set_batch job (flowgnn_group_compute and the entry points leave each engine on its last range).
 */
typedef struct flowgnn_group flowgnn_group;
int flowgnn_shard_ranges(int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, int parts, int* cuts);
int flowgnn_create_multi(int model, int n_devices, const int* device_ids, flowgnn_group** out);
int flowgnn_group_destroy(flowgnn_group* g);
int flowgnn_group_size(const flowgnn_group* g);
flowgnn_engine* flowgnn_group_engine(flowgnn_group* g, int i);
const char* flowgnn_group_last_error(const flowgnn_group* g);
int flowgnn_group_set_weights(flowgnn_group* g, int count, const float* const* tensors);
int flowgnn_group_load_weights_dir(flowgnn_group* g, const char* dir);
int flowgnn_group_set_option(flowgnn_group* g, const char* key, double value);
int flowgnn_group_set_num_tasks(flowgnn_group* g, int num_tasks);
int flowgnn_group_set_emb_dim(flowgnn_group* g, int emb_dim);
int flowgnn_group_set_model_emb_dim(flowgnn_group* g, int emb_dim);
int flowgnn_group_set_numeric_mode(flowgnn_group* g, int mode);
int flowgnn_group_set_numeric_mode_dim(flowgnn_group* g, int emb_dim, int mode);
int flowgnn_group_set_model_numeric_mode_dim(flowgnn_group* g, int emb_dim, int mode);
int flowgnn_group_set_model_numeric_mode(flowgnn_group* g, int model_id, int mode);   /* flowgnn_set_model_numeric_mode on every member */
int flowgnn_group_set_pooling(flowgnn_group* g, int mode);
int flowgnn_group_set_gin_eps(flowgnn_group* g, const float* eps);
int flowgnn_group_set_ogb_virtual_node(flowgnn_group* g, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2);
int flowgnn_group_set_ogb_virtual_node_dim(flowgnn_group* g, int emb_dim, const float* vn_embedding, const float* w1, const float* b1,
                                           const float* w2, const float* b2);
int flowgnn_group_set_gcn_virtual_node(flowgnn_group* g, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2);
int flowgnn_group_set_gcn_virtual_node_dim(flowgnn_group* g, int emb_dim, const float* vn_embedding, const float* w1, const float* b1,
                                           const float* w2, const float* b2);
int flowgnn_group_set_attention_pooling(flowgnn_group* g, int emb_dim, const float* w1, const float* b1, const float* w2);
int flowgnn_group_set_set2set_pooling(flowgnn_group* g, int emb_dim, int steps, int num_tasks, const float* w_ih, const float* w_hh,
                                      const float* b_ih, const float* b_hh, const float* head_w, const float* head_b);
int flowgnn_group_set_jk_residual(flowgnn_group* g, int emb_dim, int jk, int residual);
int flowgnn_group_set_model_jk_residual(flowgnn_group* g, int emb_dim, int jk, int residual);
int flowgnn_group_set_num_layers(flowgnn_group* g, int emb_dim, int num_layers);   /* flowgnn_set_num_layers on every member */
int flowgnn_group_set_batch(flowgnn_group* g, int num_graphs,
                            const int* nums_of_nodes, const int* nums_of_edges,
                            const int* node_feature, const int* edge_list, const int* edge_attr,
                            const float* node_eigen);
int flowgnn_group_shards(const flowgnn_group* g, int* cuts /* [size + 1] */);
int flowgnn_group_run(flowgnn_group* g);
int flowgnn_group_sync(flowgnn_group* g);
int flowgnn_group_get_results(flowgnn_group* g, float* out_host);
/* flowgnn_set_embeddings on every member; flowgnn_group_get_embeddings writes [num_graphs][dim] in job order, like flowgnn_group_get_results. */
int flowgnn_group_set_embeddings(flowgnn_group* g, int on);
int flowgnn_group_get_embeddings(flowgnn_group* g, float* out_host);
/* flowgnn_set_node_embeddings on every member; flowgnn_group_get_node_embeddings writes [N_tot][dim] in job order (the shards are contiguous graph ranges). */
int flowgnn_group_set_node_embeddings(flowgnn_group* g, int on);
int flowgnn_group_get_node_embeddings(flowgnn_group* g, float* out_host);
/* flowgnn_set_node_logits on every member; flowgnn_group_get_node_logits writes [N_tot][NUM_TASK] in job order. */
int flowgnn_group_set_node_logits(flowgnn_group* g, int on);
int flowgnn_group_get_node_logits(flowgnn_group* g, float* out_host);
/* flowgnn_set_attention on every member; flowgnn_group_get_attention writes [n_sel][E_tot][4] and [n_sel][N_tot][4] in job order
 * (either pointer may be NULL). */
int flowgnn_group_set_attention(flowgnn_group* g, int layer_mask);
int flowgnn_group_get_attention(flowgnn_group* g, float* edge_host, float* self_host);
/* set_batch + run + get_results for a batch in HOST memory, cut into size x chunks_per_engine ranges; engine i takes ranges
 * i, i + size, ... in turn, so that one engine's copies overlap the others' kernels.  out_host: [num_graphs][NUM_TASK]. */
int flowgnn_group_compute(flowgnn_group* g, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges,
                          const int* node_feature, const int* edge_list, const int* edge_attr, const float* node_eigen,
                          float* out_host, int chunks_per_engine);

/*
 * Debug / parity taps (device -> host copies; synchronise first).
 *  flowgnn_get_csr: the batched destination-major CSR built by load_graph:
 *     row_ptr[N_tot+1], src[E_tot] (global source id, ascending per row, ties in
 *     input order), eid[E_tot] (input edge index), out_deg[N_tot].
 *  flowgnn_get_h: node embeddings after the last executed stage, [N_tot][dim].
 */
int flowgnn_get_csr(flowgnn_engine* e, int* row_ptr, int* src, int* eid, int* out_deg);
int flowgnn_get_h(flowgnn_engine* e, float* h_host, int* dim);

/*
 * Per-kernel profile with HIP events on the engine's stream.
 *  flowgnn_profile_enable(e, 1) brackets every kernel launch of subsequent runs
 *  with events; flowgnn_profile_read fills, for kernel slot k < *count,
 *  total milliseconds and launch counts since enable, and the kernel names.
 */
#define FLOWGNN_MAX_PROFILE_SLOTS 32
int flowgnn_profile_enable(flowgnn_engine* e, int on);
int flowgnn_profile_read(flowgnn_engine* e, int* count, const char** names,
                         double* total_ms, long long* launches);

/*
 * Standalone aggregation kernel of layer `layer` on the resident batch (the
 * message-passing unit alone, m written to HBM): used to measure the HBM roofline
 * of the gather + segmented-sum path.  Requires a prior flowgnn_run.
 */
int flowgnn_run_aggregation_only(flowgnn_engine* e, int layer, int iters, float* avg_ms);
/*
 * Parity tap for that kernel: runs it once, on the node embeddings the last flowgnn_run left in the engine (the input
 * of the model's last stage when the readout was folded into it, the last layer's output otherwise), and copies to the
 * host the rows it read (h_in_host, [N_tot][*in_dim]) and what it wrote (agg_host, [N_tot][*agg_dim]; GIN: m + h,
 * GCN: relu(BN(...)), PNA: [mean|min|max|std] x 80, DGN: [mean | directional] x 100).  Either buffer may be NULL
 * (dims are still reported).  The next flowgnn_run rewrites everything this touches.
 */
int flowgnn_get_aggregate(flowgnn_engine* e, int layer, float* h_in_host, int* in_dim, float* agg_host, int* agg_dim);

#ifdef __cplusplus
}
#endif
#endif
