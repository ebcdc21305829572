// engine_config.hip -- the calls that configure an engine (include/flowgnn.h): NUM_TASK, width, numeric mode, pooling, eps, the two
// virtual nodes, the attention and set2set readouts, JK / residual, the depth, and their getters.  Host code only; what it shares with engine.hip
// (begin_change, use_device, kOutputs) is declared in engine_internal.h.
//
// Every setter is: its argument checks, its state checks, begin_change (or use_device + drop_graph where no device memory changes
// hands), then the engine's field and the DeviceBatch field that follows it.  The checks repeated from call to call are the helpers
// right below; the order of the checks within a call decides which refusal wins when two apply, and tests/golden/config_calls.json
// holds that order.  A new option that carries tensors follows flowgnn_set_attention_pooling: width_argument, tensor_set_on, its own
// argument checks, tensor_set_finite, its state checks, begin_change, upload_packed, its own fields.
#include "engine_internal.h"
#include "wide_attn.h"
#include "wide_s2s.h"
#include <cmath>

using namespace fg;

// a refusal: the text for flowgnn_last_error, and the status the call returns
static int refuse(flowgnn_engine* e, int status, const std::string& text) {
    e->err = text;
    return status;
}

// ------------------------------------------------------------------ the repeated checks: a refusal, or 0 = passed
static const char kWidthSetters[] = "flowgnn_set_emb_dim / flowgnn_set_model_emb_dim";

// a width argument: 100 or 300.  pna_hint: the call has a model form that takes FLOWGNN_EMB_DIM_PNA, and says so to who passes it here
static int width_argument(flowgnn_engine* e, const std::string& who, int emb_dim, bool pna_hint = false) {
    if (emb_dim == FLOWGNN_EMB_DIM_REFERENCE || emb_dim == FLOWGNN_EMB_DIM_OGB) return FLOWGNN_OK;
    e->err = who + "emb_dim is " + std::to_string(emb_dim) + "; the widths are FLOWGNN_EMB_DIM_REFERENCE (100) and FLOWGNN_EMB_DIM_OGB (300)";
    if (pna_hint && emb_dim == FLOWGNN_EMB_DIM_PNA)
        e->err += "; FLOWGNN_EMB_DIM_PNA (80) is a width of the model form alone, flowgnn_set_model_numeric_mode_dim on a FLOWGNN_MODEL_PNA engine";
    return FLOWGNN_ERR_ARG;
}

static int mode_argument(flowgnn_engine* e, const std::string& who, int mode) {
    if (mode == FLOWGNN_NUMERIC_F32 || mode == FLOWGNN_NUMERIC_Q6_10 || mode == FLOWGNN_NUMERIC_F16) return FLOWGNN_OK;
    return refuse(e, FLOWGNN_ERR_ARG, who + "mode is " + std::to_string(mode) + "; the modes are FLOWGNN_NUMERIC_F32 (0), FLOWGNN_NUMERIC_Q6_10 (1) and FLOWGNN_NUMERIC_F16 (2)");
}

// the argument's width against the engine's.  tensors: the argument is the width of the call's tensors, not a bare emb_dim
static int width_matches(flowgnn_engine* e, const std::string& who, bool tensors, int emb_dim, int width, const char* setters = kWidthSetters) {
    if (emb_dim == width) return FLOWGNN_OK;
    return refuse(e, FLOWGNN_ERR_ARG, who + (tensors ? "the tensors are " + std::to_string(emb_dim) + " wide" : "emb_dim is " + std::to_string(emb_dim)) +
                                          " and the engine's width is " + std::to_string(width) + " (" + setters + ")");
}

// A set of tensors that is given whole (on) or not at all (off), in two steps because a call may have arguments to check in between
// (set2set's steps and NUM_TASK, which size its head): all or none of them ...
struct TensorArg {
    const char* name;
    const float* p;
    size_t count;  // elements
};
template <size_t N>
static int tensor_set_on(flowgnn_engine* e, const std::string& who, const TensorArg (&t)[N], bool* on) {
    static const char* const words[] = {"no", "one", "two", "three", "four", "five", "six"};
    static_assert(N < sizeof(words) / sizeof(words[0]), "a word for the count");
    size_t given = 0;
    for (const TensorArg& a : t) given += a.p != nullptr;
    *on = given == N;
    if (given == 0 || given == N) return FLOWGNN_OK;
    return refuse(e, FLOWGNN_ERR_ARG, who + "some of the " + words[N] + " tensors are NULL and some are not (all " + words[N] + ": on, all NULL: off)");
}
// ... and, of a set that is given, every element finite: the first that is not is named
template <size_t N>
static int tensor_set_finite(flowgnn_engine* e, const std::string& who, const TensorArg (&t)[N]) {
    for (const TensorArg& a : t)
        for (size_t k = 0; k < a.count; k++)
            if (!std::isfinite(a.p[k]))
                return refuse(e, FLOWGNN_ERR_ARG, who + a.name + "[" + std::to_string(k) + "] is not finite");
    return FLOWGNN_OK;
}

// The device form of a tensor set, `bytes` of floats that `pack` writes on the host, into the engine's buffer for it.  After
// begin_change: a run in flight may still read the tensors this replaces.
template <class Pack>
static int upload_packed(flowgnn_engine* e, fg::GrowBuf& buf, size_t bytes, Pack pack) {
    std::vector<float> packed(bytes / sizeof(float));  // (floats: the parts are read as float4 pieces)
    pack(packed.data());
    EHIP_TRY(e, buf.reserve(bytes, false));
    EHIP_TRY(e, hipMemcpy(buf.p, packed.data(), bytes, hipMemcpyHostToDevice));
    return FLOWGNN_OK;
}

// What the two readouts of the 300-wide models (attention, set2set) refuse alike, once their tensors are known to be sound.  `name`:
// this readout; blob_bytes: the size of its device form at this width (0: none); other_*: the other readout, which excludes this one
static int wide_readout_state(flowgnn_engine* e, const std::string& who, const char* name, int emb_dim, size_t blob_bytes, bool other_on,
                              const char* other_name, const char* other_call) {
    if (e->model_id != FLOWGNN_MODEL_GIN && e->model_id != FLOWGNN_MODEL_GCN)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the " + name + " pooling exists for FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN only (OGB's gin, gin-virtual, gcn, gcn-virtual)");
    if (int rc = width_matches(e, who, true, emb_dim, e->emb_dim)) return rc;
    if (emb_dim != FLOWGNN_EMB_DIM_OGB || blob_bytes == 0)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "only the 300-wide models have this readout (the 100-wide graph-resident kernels fold the mean into their last layer): "
                                                        "flowgnn_set_emb_dim / flowgnn_set_model_emb_dim(e, 300) first");
    if (e->pooling != FLOWGNN_POOL_MEAN)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the pooling is not the mean (flowgnn_set_pooling), and this readout replaces the pooling: set FLOWGNN_POOL_MEAN first");
    if (e->nlog_on)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "node logits are on (flowgnn_set_node_logits), and under this readout a graph's logit is no mean of per-node terms");
    if (other_on)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the " + other_name + " pooling is on (" + other_call + "), and the two readouts exclude each other: turn that one off first");
    return FLOWGNN_OK;
}

extern "C" {

int flowgnn_set_num_tasks(flowgnn_engine* e, int num_tasks) {
    if (!e || num_tasks < 1) return FLOWGNN_ERR_ARG;
    if (e->s2s_steps && num_tasks != e->num_tasks)  // (the readout's own head has NUM_TASK rows)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_num_tasks: the set2set pooling is on (flowgnn_set_set2set_pooling), and its head has " + std::to_string(e->num_tasks) +
                                                  " tasks, not " + std::to_string(num_tasks) + ": turn it off, change NUM_TASK, set it again");
    ENGINE_TRY(e, begin_change(e));
    const int rc = e->model->set_num_tasks(num_tasks);
    if (rc) return refuse(e, rc, "flowgnn_set_num_tasks: this model's readout has a single task (multi-task readout exists for GIN / GIN-VN / GCN)");
    e->num_tasks = num_tasks;
    e->batch_ready = false;  // the result buffer is sized by the batch: set the batch again
    e->ran = false;
    return FLOWGNN_OK;
}

int flowgnn_num_tasks(const flowgnn_engine* e) { return e ? e->num_tasks : -1; }

// The width is the model OBJECT: GinModel (gin.hip) / GcnModel (gcn.hip) at 100, the per-layer models of gin_wide.hip / gcn_wide.hip at
// 300.  The call swaps it; everything the old object held (weights) goes with it, and everything sized by the width (h, the embeddings,
// the node embeddings) with the batch.  `fn`: the caller (flowgnn_set_emb_dim: GIN; flowgnn_set_model_emb_dim: GIN and GCN).
static int set_width(flowgnn_engine* e, const char* fn, int emb_dim) {
    const std::string who = std::string(fn) + ": ";
    const bool gcn = e->model_id == FLOWGNN_MODEL_GCN;
    if (emb_dim == e->emb_dim) return FLOWGNN_OK;
    if (e->numeric_mode != FLOWGNN_NUMERIC_F32)  // (either direction: the mode is the model object's, and the call swaps the object)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED,
                      who + (emb_dim != FLOWGNN_EMB_DIM_REFERENCE
                                 ? "a numeric mode other than FLOWGNN_NUMERIC_F32 is on (flowgnn_set_numeric_mode), and the width changes in "
                                   "FLOWGNN_NUMERIC_F32 only: width 300 has no fixed-point kernels, and the f16 mode at width 300 is set at that width, through "
                                   "flowgnn_set_numeric_mode_dim (GIN) or flowgnn_set_model_numeric_mode_dim (GCN)"
                                 : "a numeric mode other than FLOWGNN_NUMERIC_F32 is on at width 300 (flowgnn_set_numeric_mode_dim / flowgnn_set_model_numeric_mode_dim), and the width changes "
                                   "in FLOWGNN_NUMERIC_F32 only: set that mode, change the width, set the numeric mode again"));
    const std::string not_that_wide = std::to_string(e->emb_dim) + " wide, not " + std::to_string(emb_dim) + ": turn it off, change the width, set it again";
    if (e->ogb_vn_on)  // (either direction: the tensors belong to a width -- turn it off, change the width, set it again)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "OGB's virtual node is on (" + (gcn ? "flowgnn_set_gcn_virtual_node / flowgnn_set_gcn_virtual_node_dim" : "flowgnn_set_ogb_virtual_node / flowgnn_set_ogb_virtual_node_dim") +
                                                  "), and its tensors are " + not_that_wide);
    if (e->attn_pool_on)  // (the same rule: the gate's tensors belong to a width)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the attention pooling is on (flowgnn_set_attention_pooling), and its tensors are " + not_that_wide);
    if (e->s2s_steps)  // (and the same again)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the set2set pooling is on (flowgnn_set_set2set_pooling), and its tensors are " + not_that_wide);
    if (e->jk != FLOWGNN_JK_LAST || e->residual)  // (on means width 300: the call asks for 100, which has no instance)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "JK sum or the residual is on (" + (gcn ? "flowgnn_set_model_jk_residual" : "flowgnn_set_jk_residual") + "), and only the 300-wide " +
                                                  (gcn ? "GCN" : "GIN") + " has those instances, not width " + std::to_string(emb_dim) +
                                                  ": turn it off (FLOWGNN_JK_LAST, 0), then change the width");
    if (e->num_layers != FLOWGNN_NUM_LAYERS_DEFAULT)  // (not 5 means width 300: the call asks for 100, whose kernels are five layers deep)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the depth is " + std::to_string(e->num_layers) + " (flowgnn_set_num_layers), and the " + std::to_string(emb_dim) +
                                                  "-wide kernels are five layers deep: flowgnn_set_num_layers(e, " + std::to_string(e->emb_dim) + ", 5) first, then change the width");
    ENGINE_TRY(e, begin_change(e));
    Model* m = gcn ? (emb_dim == FLOWGNN_EMB_DIM_REFERENCE ? make_gcn_model() : make_gcn_wide_model(emb_dim))
                   : (emb_dim == FLOWGNN_EMB_DIM_REFERENCE ? make_gin_model(false) : make_gin_wide_model(emb_dim));
    if (!m) return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "no model of this width");
    m->configure(e->opts);
    if (int rc = m->set_num_tasks(e->num_tasks)) {
        delete m;
        return refuse(e, rc, who + "the model of this width does not take the engine's NUM_TASK");
    }
    delete e->model;  // (the stream is idle: begin_change)
    e->model = m;
    e->emb_dim = emb_dim;
    e->free_batch();  // h, scratch and the outputs are sized by the width: the batch has to be set again, and so have the weights
    e->batch_ready = false;
    e->ran = false;
    e->force_exact = false;
    e->db.tap = nullptr;
    for (const Output& o : kOutputs) {
        (e->*o.slot).user = (e->*o.slot).last = nullptr;
        e->db.*o.field = nullptr;
    }
    return FLOWGNN_OK;
}

int flowgnn_set_emb_dim(flowgnn_engine* e, int emb_dim) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (emb_dim != FLOWGNN_EMB_DIM_REFERENCE && emb_dim != FLOWGNN_EMB_DIM_OGB)
        return refuse(e, FLOWGNN_ERR_ARG, "flowgnn_set_emb_dim: the widths are FLOWGNN_EMB_DIM_REFERENCE (100) and FLOWGNN_EMB_DIM_OGB (300)");
    if (e->model_id != FLOWGNN_MODEL_GIN)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_emb_dim: the width is a choice of FLOWGNN_MODEL_GIN alone in this call (GIN-VN and the other models have the reference's width only; "
                                                  "GCN's width goes through flowgnn_set_model_emb_dim)");
    return set_width(e, "flowgnn_set_emb_dim", emb_dim);
}

// The call that names no model: GIN exactly as flowgnn_set_emb_dim (the same code path, state and bits), GCN between GcnModel and
// gcn_wide.hip's model.
int flowgnn_set_model_emb_dim(flowgnn_engine* e, int emb_dim) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (emb_dim != FLOWGNN_EMB_DIM_REFERENCE && emb_dim != FLOWGNN_EMB_DIM_OGB)
        return refuse(e, FLOWGNN_ERR_ARG, "flowgnn_set_model_emb_dim: the widths are FLOWGNN_EMB_DIM_REFERENCE (100) and FLOWGNN_EMB_DIM_OGB (300)");
    if (e->model_id != FLOWGNN_MODEL_GIN && e->model_id != FLOWGNN_MODEL_GCN)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_model_emb_dim: the width is a choice of FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN (the other models have the reference's width only)");
    return set_width(e, e->model_id == FLOWGNN_MODEL_GIN ? "flowgnn_set_emb_dim" : "flowgnn_set_model_emb_dim", emb_dim);
}

int flowgnn_emb_dim(const flowgnn_engine* e) { return e ? e->emb_dim : -1; }
}  // extern "C"

// ------------------------------------------------------------------ numeric mode
// By which public call a request reached set_numeric_mode.  The calls forward to one another (the model form of the width-carrying call
// is the plain one on every engine but GCN and PNA; the call that names the model is the model form at the engine's width on every
// engine but DGN), and the route is the LAST call of that chain: the one whose rules apply.
enum class ModeRoute {
    NumericMode,             // flowgnn_set_numeric_mode
    NumericModeDim,          // flowgnn_set_numeric_mode_dim, with the engine's width (100 or 300)
    ModelNumericModeDim,     // flowgnn_set_model_numeric_mode_dim on a GCN engine, with the engine's width
    ModelNumericModeDimPna,  // flowgnn_set_model_numeric_mode_dim(e, FLOWGNN_EMB_DIM_PNA, ..) on a PNA engine
    ModelNumericMode,        // flowgnn_set_model_numeric_mode(e, FLOWGNN_MODEL_DGN, ..) on a DGN engine
};

// THE rule of which call reaches FLOWGNN_NUMERIC_F16 on which engine.  Every f16 path after the first (GIN / GIN-VN at width 100) came
// with a call of its own, so that the calls that existed before keep answering what they answered: gin_wide_f16.hip (DESIGN.md section
// 4.22), gcn_wide_f16.hip (4.27), pna_f16.hip (4.28), dgn_f16.hip (4.29).
static bool route_reaches_f16(const flowgnn_engine* e, ModeRoute route) {
    const bool wide = off_default_width(e);
    switch (e->model_id) {
        case FLOWGNN_MODEL_GIN: return !wide || route != ModeRoute::NumericMode;         // at 300: the calls that carry the width
        case FLOWGNN_MODEL_GCN: return !wide || route == ModeRoute::ModelNumericModeDim;  // at 300: the model form only (at 100 GcnModel has no f16 mode, and says so)
        case FLOWGNN_MODEL_PNA: return route == ModeRoute::ModelNumericModeDimPna;
        case FLOWGNN_MODEL_DGN: return route == ModeRoute::ModelNumericMode;
        default: return true;  // GIN-VN: any call; GAT: the model object has no such mode, and says so
    }
}

// An engine at width 300 has FLOWGNN_NUMERIC_F32 and, by the route above, FLOWGNN_NUMERIC_F16: what each call says to anything else
static const char* no_such_mode_at_300(ModeRoute route) {
    switch (route) {
        case ModeRoute::NumericMode:
            return "flowgnn_set_numeric_mode: the engine's width is 300 (flowgnn_set_emb_dim / flowgnn_set_model_emb_dim), which has no fixed-point "
                   "kernels; GIN's f16 mode at that width goes through flowgnn_set_numeric_mode_dim, GCN's through flowgnn_set_model_numeric_mode_dim";
        case ModeRoute::NumericModeDim:
            return "flowgnn_set_numeric_mode_dim: at width 300 the modes are FLOWGNN_NUMERIC_F32 and, for FLOWGNN_MODEL_GIN, FLOWGNN_NUMERIC_F16; "
                   "there are no fixed-point kernels at that width, and GCN's f16 mode at that width goes through "
                   "flowgnn_set_model_numeric_mode_dim";
        default:
            return "flowgnn_set_model_numeric_mode_dim: at width 300 the modes are FLOWGNN_NUMERIC_F32 and FLOWGNN_NUMERIC_F16; there are no "
                   "fixed-point kernels at that width";
    }
}

// The four public calls at the engine's width, once their own arguments are checked.  At width 100 the routes differ in nothing but
// the f16 rule.
static int set_numeric_mode(flowgnn_engine* e, int mode, ModeRoute route) {
    if (mode == FLOWGNN_NUMERIC_F16 && !route_reaches_f16(e, route))
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED,
                      e->model_id == FLOWGNN_MODEL_DGN ? "flowgnn_set_numeric_mode: DGN's f16 mode goes through the call that names the model: "
                                                         "flowgnn_set_model_numeric_mode(e, FLOWGNN_MODEL_DGN, FLOWGNN_NUMERIC_F16)"
                      : e->model_id == FLOWGNN_MODEL_PNA ? "flowgnn_set_numeric_mode: PNA's f16 mode goes through the call that carries the model, with the model's true width: "
                                                           "flowgnn_set_model_numeric_mode_dim(e, FLOWGNN_EMB_DIM_PNA (80), FLOWGNN_NUMERIC_F16)"
                                                         : no_such_mode_at_300(route));
    for (const Output& o : kOutputs)
        if (mode == FLOWGNN_NUMERIC_Q6_10 && o.no_fixed_point && is_on(e, o))
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, o.no_fixed_point);
    if (mode != FLOWGNN_NUMERIC_F32 && mode != FLOWGNN_NUMERIC_F16 && off_default_width(e))
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, no_such_mode_at_300(route));
    if (mode == FLOWGNN_NUMERIC_Q6_10 && e->pooling != FLOWGNN_POOL_MEAN)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_numeric_mode: the pooling is not the mean (flowgnn_set_pooling), and the fixed-point readout is the reference's mean");
    if (mode == FLOWGNN_NUMERIC_Q6_10 && e->gin_eps_on)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_numeric_mode: a trained eps is on (flowgnn_set_gin_eps), and the fixed-point arithmetic is the reference's, which has no eps");
    if (mode == FLOWGNN_NUMERIC_Q6_10 && e->ogb_vn_on)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_numeric_mode: OGB's virtual node is on (flowgnn_set_ogb_virtual_node / flowgnn_set_gcn_virtual_node), and the fixed-point arithmetic is the reference's, which has no such model");
    e->drop_graph();
    const int rc = e->model->set_numeric_mode(mode);
    if (!rc) e->numeric_mode = mode;
    if (rc) e->err = "flowgnn_set_numeric_mode: unknown mode, a mode this model does not have (f16: GIN / GIN-VN only), or the fixed-point "
                     "readout is single-task and NUM_TASK != 1";
    return rc;
}

// (flowgnn_emb_dim is the model's own figure for the models without a choice of width -- GAT's 16; their width for these calls is 100)
static int numeric_mode_width(const flowgnn_engine* e) { return off_default_width(e) ? e->emb_dim : FLOWGNN_EMB_DIM_REFERENCE; }

// The calls that carry the width: emb_dim must be the engine's.  100 IS flowgnn_set_numeric_mode (the same state, kernels and bits).
static int set_numeric_mode_dim(flowgnn_engine* e, const char* fn, int emb_dim, int mode, ModeRoute route) {
    const std::string who = std::string(fn) + ": ";
    if (int rc = width_argument(e, who, emb_dim, true)) return rc;
    if (int rc = mode_argument(e, who, mode)) return rc;
    if (int rc = width_matches(e, who, false, emb_dim, numeric_mode_width(e))) return rc;
    return set_numeric_mode(e, mode, route);
}

extern "C" {

int flowgnn_set_numeric_mode(flowgnn_engine* e, int mode) {
    if (!e) return FLOWGNN_ERR_ARG;
    return set_numeric_mode(e, mode, ModeRoute::NumericMode);
}

int flowgnn_set_numeric_mode_dim(flowgnn_engine* e, int emb_dim, int mode) {
    if (!e) return FLOWGNN_ERR_ARG;
    return set_numeric_mode_dim(e, "flowgnn_set_numeric_mode_dim", emb_dim, mode, ModeRoute::NumericModeDim);
}

// The call that names no model, as flowgnn_set_model_emb_dim is for the width: its own on a GCN engine and, with PNA's true width, on a
// PNA engine (F32, Q6_10 -- the plain call's -- and F16); on every other engine it is the call above.
int flowgnn_set_model_numeric_mode_dim(flowgnn_engine* e, int emb_dim, int mode) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (e->model_id == FLOWGNN_MODEL_PNA && emb_dim == FLOWGNN_EMB_DIM_PNA) {
        if (int rc = mode_argument(e, "flowgnn_set_model_numeric_mode_dim: ", mode)) return rc;
        return set_numeric_mode(e, mode, ModeRoute::ModelNumericModeDimPna);
    }
    if (e->model_id != FLOWGNN_MODEL_GCN) return flowgnn_set_numeric_mode_dim(e, emb_dim, mode);
    return set_numeric_mode_dim(e, "flowgnn_set_model_numeric_mode_dim", emb_dim, mode, ModeRoute::ModelNumericModeDim);
}

// The call that names the model: one call that reaches every mode any engine has.  On a DGN engine (whose width is the reference's 100,
// so no width of its own to enter through) it takes F32, Q6_10 and F16; on every other engine it is flowgnn_set_model_numeric_mode_dim
// at that engine's own current width.
int flowgnn_set_model_numeric_mode(flowgnn_engine* e, int model_id, int mode) {
    if (!e) return FLOWGNN_ERR_ARG;
    static const char* const names[] = {"FLOWGNN_MODEL_GIN", "FLOWGNN_MODEL_GIN_VN", "FLOWGNN_MODEL_GCN", "FLOWGNN_MODEL_GAT", "FLOWGNN_MODEL_PNA", "FLOWGNN_MODEL_DGN"};
    auto name = [&](int m) { return std::to_string(m) + " (" + ((m >= 0 && m < 6) ? names[m] : "no model") + ")"; };
    if (model_id != e->model_id)
        return refuse(e, FLOWGNN_ERR_ARG, "flowgnn_set_model_numeric_mode: model_id is " + name(model_id) + " and the engine's model is " + name(e->model_id));
    if (e->model_id == FLOWGNN_MODEL_DGN) {
        if (int rc = mode_argument(e, "flowgnn_set_model_numeric_mode: ", mode)) return rc;
        return set_numeric_mode(e, mode, ModeRoute::ModelNumericMode);
    }
    const int width = e->model_id == FLOWGNN_MODEL_PNA ? FLOWGNN_EMB_DIM_PNA : numeric_mode_width(e);
    return flowgnn_set_model_numeric_mode_dim(e, width, mode);
}

// ------------------------------------------------------------------ pooling, eps
int flowgnn_set_pooling(flowgnn_engine* e, int mode) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (mode != FLOWGNN_POOL_MEAN && mode != FLOWGNN_POOL_SUM && mode != FLOWGNN_POOL_MAX)
        return refuse(e, FLOWGNN_ERR_ARG, "flowgnn_set_pooling: the modes are FLOWGNN_POOL_MEAN (0), FLOWGNN_POOL_SUM (1) and FLOWGNN_POOL_MAX (2)");
    if (mode != FLOWGNN_POOL_MEAN && (e->model_id == FLOWGNN_MODEL_PNA || e->model_id == FLOWGNN_MODEL_DGN))
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_pooling: PNA and DGN read the pooled vector through an MLP head that was trained on the mean");
    if (mode != FLOWGNN_POOL_MEAN && e->numeric_mode == FLOWGNN_NUMERIC_Q6_10)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_pooling: the fixed-point readout (FLOWGNN_NUMERIC_Q6_10) is the reference's mean");
    if (mode != FLOWGNN_POOL_MEAN && e->nlog_on)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_pooling: node logits are on, and they are the terms whose mean is the logit");
    if (mode != FLOWGNN_POOL_MEAN && e->attn_pool_on)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_pooling: the attention pooling is on (flowgnn_set_attention_pooling), a readout of its own; beside it the mean is the only accepted value");
    if (mode != FLOWGNN_POOL_MEAN && e->s2s_steps)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_pooling: the set2set pooling is on (flowgnn_set_set2set_pooling), a readout of its own; beside it the mean is the only accepted value");
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();  // a recorded launch sequence is that of the other mode
    e->pooling = mode;
    e->db.pooling = mode;  // (launches are stream-ordered: the mode matters to those enqueued after this call)
    return FLOWGNN_OK;
}

int flowgnn_pooling(const flowgnn_engine* e) { return e ? e->pooling : -1; }

int flowgnn_set_gin_eps(flowgnn_engine* e, const float* eps) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (e->model_id != FLOWGNN_MODEL_GIN && e->model_id != FLOWGNN_MODEL_GIN_VN)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_gin_eps: only GIN and GIN-VN have the (1 + eps) self term");
    if (eps) {
        for (int l = 0; l < e->num_layers; l++)
            if (!std::isfinite(eps[l]))
                return refuse(e, FLOWGNN_ERR_ARG, "flowgnn_set_gin_eps: eps[" + std::to_string(l) + "] is not finite");
        if (e->numeric_mode == FLOWGNN_NUMERIC_Q6_10)
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, "flowgnn_set_gin_eps: the fixed-point arithmetic (FLOWGNN_NUMERIC_Q6_10) is the reference's, which has no eps");
    }
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();  // a recorded launch sequence is that of the other state (or carries the other values in its argument blocks)
    e->gin_eps_on = eps != nullptr;
    e->db.gin_eps_on = e->gin_eps_on;  // (launches are stream-ordered: the values matter to those enqueued after this call)
    for (int l = 0; l < FLOWGNN_MAX_NUM_LAYERS; l++) {  // (the caller's array has flowgnn_num_layers(e) floats; beyond them: zeros)
        e->gin_eps[l] = (eps && l < e->num_layers) ? eps[l] : 0.0f;
        e->db.gin_self_scale[l] = (float)(1.0f + e->gin_eps[l]);
    }
    return FLOWGNN_OK;
}

int flowgnn_gin_eps(const flowgnn_engine* e, float* eps_out) {
    if (!e) return -1;
    if (eps_out)
        for (int l = 0; l < e->num_layers; l++) eps_out[l] = e->gin_eps[l];
    return e->gin_eps_on ? 1 : 0;
}
}  // extern "C"

// ------------------------------------------------------------------ OGB's virtual node
// flowgnn_set_ogb_virtual_node (GIN) and flowgnn_set_gcn_virtual_node (GCN): the same five tensors, the same checks and the same engine
// state -- an engine is one model, so one of the two calls is refused on it.  `fn`: the caller.  `dim`: the tensors' width D (hidden
// width 2 D) -- 100 in the two calls without a width argument.  The device form is the model object's (Model::ogb_vn_pack): gin_ogbvn.h's
// at width 100, gin_wide.hip's own at 300.
static int set_virtual_node(flowgnn_engine* e, const char* fn, const float* vn_embedding, const float* w1, const float* b1, const float* w2,
                            const float* b2, int dim) {
    const std::string who = std::string(fn) + ": ";
    const size_t D = (size_t)dim, H = 2 * D, L = (size_t)e->num_layers - 1;  // (FLOWGNN_OGB_VN_LAYERS unless flowgnn_set_num_layers said otherwise)
    const TensorArg t[5] = {{"vn_embedding", vn_embedding, D}, {"w1", w1, L * H * D}, {"b1", b1, L * H}, {"w2", w2, L * D * H}, {"b2", b2, L * D}};
    bool on;
    if (int rc = tensor_set_on(e, who, t, &on)) return rc;
    if (on) {
        if (int rc = tensor_set_finite(e, who, t)) return rc;
        if (e->numeric_mode == FLOWGNN_NUMERIC_Q6_10)
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the fixed-point arithmetic (FLOWGNN_NUMERIC_Q6_10) is the reference's, which has no such model");
        // (the model object has this width and a device form for the tensors; refused before anything changes)
        if (e->model->emb_dim() != dim || e->model->ogb_vn_blob_bytes() == 0)
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "this model has no such kernel");
    }
    ENGINE_TRY(e, begin_change(e));
    if (on)
        if (int rc = upload_packed(e, e->ogb_vn, e->model->ogb_vn_blob_bytes(), [&](float* dst) { e->model->ogb_vn_pack(vn_embedding, w1, b1, w2, b2, dst); }))
            return rc;
    const int rc = e->model_id == FLOWGNN_MODEL_GCN ? e->model->set_gcn_virtual_node(on ? vn_embedding : nullptr) : e->model->set_ogb_virtual_node(on);
    if (rc) return refuse(e, rc, who + "this model has no such kernel");
    e->ogb_vn_on = on;
    e->db.ogb_vn = on ? (const float*)e->ogb_vn.p : nullptr;  // (launches are stream-ordered: it matters to those enqueued after this call)
    return FLOWGNN_OK;
}

// What tells GIN's pair of calls from GCN's: the checks in front of set_virtual_node are the same, in the same order.
struct VnCalls {
    int model_id;                // the one model the calls serve
    const char* fn[2];           // the call without a width, and the one that carries it
    const char* width_call;      // what sets that model's width
    const char* wrong_model[2];  // the refusal on an engine of another model, per call ...
    const char* gcn_hint;        // ... and what a GCN engine is told besides
};
static const VnCalls kVnGin = {FLOWGNN_MODEL_GIN,
                               {"flowgnn_set_ogb_virtual_node", "flowgnn_set_ogb_virtual_node_dim"},
                               "flowgnn_set_emb_dim",
                               {": OGB's virtual node exists for GIN only (GIN-VN is the reference's augmentation, a different model)",
                                ": OGB's virtual node exists for GIN only (GIN-VN is the reference's augmentation, a different model)"},
                               "; GCN has a call of its own, flowgnn_set_gcn_virtual_node"};
static const VnCalls kVnGcn = {FLOWGNN_MODEL_GCN,
                               {"flowgnn_set_gcn_virtual_node", "flowgnn_set_gcn_virtual_node_dim"},
                               "flowgnn_set_model_emb_dim",
                               {": this call is OGB's gcn-virtual, for GCN only (GIN: flowgnn_set_ogb_virtual_node)",
                                ": this call is OGB's gcn-virtual, for GCN only (GIN: flowgnn_set_ogb_virtual_node_dim)"},
                               ""};

static int vn_wrong_model(flowgnn_engine* e, const VnCalls& c, int call) {  // call: index into VnCalls::fn
    e->err = std::string(c.fn[call]) + c.wrong_model[call];
    if (e->model_id == FLOWGNN_MODEL_GCN) e->err += c.gcn_hint;
    return FLOWGNN_ERR_UNSUPPORTED;
}

// the calls without a width: the tensors are 100 wide
static int set_virtual_node_ref(flowgnn_engine* e, const VnCalls& c, const float* vn_embedding, const float* w1, const float* b1, const float* w2,
                                const float* b2) {
    if (!e) return FLOWGNN_ERR_ARG;
    if (e->model_id != c.model_id) return vn_wrong_model(e, c, 0);
    if (off_default_width(e) && (vn_embedding || w1 || b1 || w2 || b2))
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, std::string(c.fn[0]) + ": the engine's width is 300 (" + c.width_call + "), and the virtual node's tensors are 100 wide "
                 "in this call; 300-wide tensors go through " + c.fn[1]);
    return set_virtual_node(e, c.fn[0], vn_embedding, w1, b1, w2, b2, FLOWGNN_EMB_DIM_REFERENCE);
}

// The calls that carry the width.  emb_dim 100 IS the call above (the same state, kernels and bits); 300 is gin_wide.hip's virtual node
//  or gcn_wide.hip's (section 4.19).  All five NULL: off, whatever the engine's width (no tensor is read).
static int set_virtual_node_dim(flowgnn_engine* e, const VnCalls& c, int emb_dim, const float* vn_embedding, const float* w1, const float* b1,
                                const float* w2, const float* b2) {
    if (!e) return FLOWGNN_ERR_ARG;
    const std::string who = std::string(c.fn[1]) + ": ";
    if (int rc = width_argument(e, who, emb_dim)) return rc;
    if (e->model_id != c.model_id) return vn_wrong_model(e, c, 1);
    if (vn_embedding || w1 || b1 || w2 || b2)
        if (int rc = width_matches(e, who, true, emb_dim, e->emb_dim, c.width_call)) return rc;
    return set_virtual_node(e, c.fn[1], vn_embedding, w1, b1, w2, b2, emb_dim);
}

extern "C" {

int flowgnn_set_ogb_virtual_node(flowgnn_engine* e, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2) {
    return set_virtual_node_ref(e, kVnGin, vn_embedding, w1, b1, w2, b2);
}

int flowgnn_set_ogb_virtual_node_dim(flowgnn_engine* e, int emb_dim, const float* vn_embedding, const float* w1, const float* b1, const float* w2,
                                     const float* b2) {
    return set_virtual_node_dim(e, kVnGin, emb_dim, vn_embedding, w1, b1, w2, b2);
}

int flowgnn_set_gcn_virtual_node(flowgnn_engine* e, const float* vn_embedding, const float* w1, const float* b1, const float* w2, const float* b2) {
    return set_virtual_node_ref(e, kVnGcn, vn_embedding, w1, b1, w2, b2);
}

int flowgnn_set_gcn_virtual_node_dim(flowgnn_engine* e, int emb_dim, const float* vn_embedding, const float* w1, const float* b1, const float* w2,
                                     const float* b2) {
    return set_virtual_node_dim(e, kVnGcn, emb_dim, vn_embedding, w1, b1, w2, b2);
}

int flowgnn_gcn_virtual_node(const flowgnn_engine* e) { return e ? (e->ogb_vn_on && e->model_id == FLOWGNN_MODEL_GCN ? 1 : 0) : -1; }

int flowgnn_ogb_virtual_node(const flowgnn_engine* e) { return e ? (e->ogb_vn_on && e->model_id == FLOWGNN_MODEL_GIN ? 1 : 0) : -1; }

// ------------------------------------------------------------------ the readouts of the 300-wide models
// OGB's graph_pooling="attention" (DESIGN.md section 4.20): the gate's three tensors in the device form of wide_attn.h, one device
// buffer owned by the engine.  All three NULL: off, at any width and for any model.
int flowgnn_set_attention_pooling(flowgnn_engine* e, int emb_dim, const float* w1, const float* b1, const float* w2) {
    if (!e) return FLOWGNN_ERR_ARG;
    const std::string who = "flowgnn_set_attention_pooling: ";
    if (int rc = width_argument(e, who, emb_dim)) return rc;
    const size_t D = (size_t)emb_dim, H = 2 * D;
    const TensorArg t[3] = {{"w1", w1, H * D}, {"b1", b1, H}, {"w2", w2, H}};
    bool on;
    if (int rc = tensor_set_on(e, who, t, &on)) return rc;
    if (on) {
        if (int rc = tensor_set_finite(e, who, t)) return rc;
        if (int rc = wide_readout_state(e, who, "attention", emb_dim, fg::attn_pool_blob_bytes(emb_dim), e->s2s_steps != 0, "set2set", "flowgnn_set_set2set_pooling"))
            return rc;
    }
    ENGINE_TRY(e, begin_change(e));
    if (on)
        if (int rc = upload_packed(e, e->attn_pool, fg::attn_pool_blob_bytes(emb_dim), [&](float* dst) { fg::attn_pool_blob_pack(emb_dim, w1, b1, w2, dst); }))
            return rc;
    e->attn_pool_on = on;
    e->db.attn_pool = on ? e->attn_pool.p : nullptr;  // (launches are stream-ordered: it matters to those enqueued after this call)
    return FLOWGNN_OK;
}

int flowgnn_attention_pooling(const flowgnn_engine* e) { return e ? (e->attn_pool_on ? 1 : 0) : -1; }

// OGB's graph_pooling="set2set" (DESIGN.md section 4.23): the LSTM's four tensors and the head's two in the device form of wide_s2s.h,
// one device buffer owned by the engine.  All six NULL: off, at any width and for any model.
int flowgnn_set_set2set_pooling(flowgnn_engine* e, int emb_dim, int steps, int num_tasks, const float* w_ih, const float* w_hh, const float* b_ih,
                                const float* b_hh, const float* head_w, const float* head_b) {
    if (!e) return FLOWGNN_ERR_ARG;
    const std::string who = "flowgnn_set_set2set_pooling: ";
    if (int rc = width_argument(e, who, emb_dim)) return rc;
    const size_t D = (size_t)emb_dim, T = (size_t)(num_tasks > 0 ? num_tasks : 0);
    const TensorArg t[6] = {{"w_ih", w_ih, 4 * D * 2 * D}, {"w_hh", w_hh, 4 * D * D}, {"b_ih", b_ih, 4 * D}, {"b_hh", b_hh, 4 * D}, {"head_w", head_w, T * 2 * D}, {"head_b", head_b, T}};
    bool on;
    if (int rc = tensor_set_on(e, who, t, &on)) return rc;
    if (on) {
        if (steps < 1 || steps > FLOWGNN_SET2SET_MAX_STEPS)
            return refuse(e, FLOWGNN_ERR_ARG, who + "steps is " + std::to_string(steps) + "; the processing steps are 1 .. " + std::to_string(FLOWGNN_SET2SET_MAX_STEPS) + " (OGB: 2)");
        if (num_tasks < 1 || num_tasks != e->num_tasks)
            return refuse(e, FLOWGNN_ERR_ARG, who + "head_w has " + std::to_string(num_tasks) + " tasks and the engine's NUM_TASK is " + std::to_string(e->num_tasks) +
                     " (flowgnn_set_num_tasks)");
        if (int rc = tensor_set_finite(e, who, t)) return rc;
        if (int rc = wide_readout_state(e, who, "set2set", emb_dim, fg::s2s_blob_bytes(emb_dim, num_tasks), e->attn_pool_on, "attention", "flowgnn_set_attention_pooling"))
            return rc;
        if (e->emb_on)
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "graph embeddings are on (flowgnn_set_embeddings), and the vector this readout's head reads is " + std::to_string(2 * emb_dim) +
                     " wide where every embeddings buffer is " + std::to_string(emb_dim) + " wide");
    }
    ENGINE_TRY(e, begin_change(e));
    if (on)
        if (int rc = upload_packed(e, e->s2s, fg::s2s_blob_bytes(emb_dim, num_tasks),
                                   [&](float* dst) { fg::s2s_blob_pack(emb_dim, num_tasks, w_ih, w_hh, b_ih, b_hh, head_w, head_b, dst); }))
            return rc;
    e->s2s_steps = on ? steps : 0;
    e->db.s2s = on ? e->s2s.p : nullptr;  // (launches are stream-ordered: it matters to those enqueued after this call)
    e->db.s2s_steps = e->s2s_steps;
    return FLOWGNN_OK;
}

int flowgnn_set2set_pooling(const flowgnn_engine* e) { return e ? e->s2s_steps : -1; }
}  // extern "C"

// ------------------------------------------------------------------ the depth
// OGB's num_layer for GIN and GCN at width 300: the model object's loop bound.  The sequence of
// flowgnn_set_num_tasks: begin_change, the model drops its weights, the batch has to be set again.
extern "C" {

int flowgnn_set_num_layers(flowgnn_engine* e, int emb_dim, int num_layers) {
    if (!e) return FLOWGNN_ERR_ARG;
    const std::string who = "flowgnn_set_num_layers: ";
    if (num_layers < FLOWGNN_MIN_NUM_LAYERS || num_layers > FLOWGNN_MAX_NUM_LAYERS)
        return refuse(e, FLOWGNN_ERR_ARG, who + "num_layers is " + std::to_string(num_layers) + "; the depths are " + std::to_string(FLOWGNN_MIN_NUM_LAYERS) + " .. " +
                                              std::to_string(FLOWGNN_MAX_NUM_LAYERS) + " (OGB's GNN_node raises below 2; FLOWGNN_MAX_NUM_LAYERS is the size of this ABI's per-layer arrays)");
    if (int rc = width_argument(e, who, emb_dim)) return rc;
    if (e->model_id != FLOWGNN_MODEL_GIN && e->model_id != FLOWGNN_MODEL_GCN) {
        if (num_layers == e->num_layers) return FLOWGNN_OK;  // (5: what every engine is)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the depth is a choice of FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN at width 300 (OGB's gin, gin-virtual, gcn, gcn-virtual); "
                                                        "every other model is five layers deep");
    }
    if (int rc = width_matches(e, who, false, emb_dim, e->emb_dim)) return rc;
    if (num_layers == e->num_layers) return FLOWGNN_OK;
    if (e->numeric_mode == FLOWGNN_NUMERIC_Q6_10)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "the fixed-point arithmetic (FLOWGNN_NUMERIC_Q6_10) is the reference's, which is five layers deep");
    if (emb_dim != FLOWGNN_EMB_DIM_OGB)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "only the 300-wide models have a depth other than 5 (the graph-resident and the 100-wide per-layer kernels are five layers deep): "
                                                        "flowgnn_set_emb_dim / flowgnn_set_model_emb_dim(e, 300) first");
    const std::string not_that_deep = std::to_string(e->num_layers) + " layers, not " + std::to_string(num_layers) + ": turn it off, change the depth, set it again";
    if (e->gin_eps_on)  // (the tensors belong to a depth, as the virtual node's belong to a width in set_width)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "a trained eps is on (flowgnn_set_gin_eps), and its values are those of " + not_that_deep);
    if (e->ogb_vn_on)
        return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "OGB's virtual node is on (" + (e->model_id == FLOWGNN_MODEL_GCN ? "flowgnn_set_gcn_virtual_node_dim" : "flowgnn_set_ogb_virtual_node_dim") +
                                                  "), and its tensors are those of " + not_that_deep);
    ENGINE_TRY(e, begin_change(e));
    const int rc = e->model->set_num_layers(num_layers);
    if (rc) return refuse(e, rc, who + "this model is five layers deep");
    e->num_layers = num_layers;
    e->batch_ready = false;  // as flowgnn_set_num_tasks: weights and batch are set again
    e->ran = false;
    e->force_exact = false;
    return FLOWGNN_OK;
}

int flowgnn_num_layers(const flowgnn_engine* e) { return e ? e->num_layers : -1; }
}  // extern "C"

// ------------------------------------------------------------------ JK / residual
// OGB's JK="sum" and residual=True at width 300: GIN and, through the model form of the call, GCN (section
// 4.25).  No tensors: the setting is two integers of the engine's, like the pooling mode, and db.jk / db.residual carry it to
// GinWideModel::forward / GcnWideModel::forward.  (FLOWGNN_JK_LAST, 0) is the default state and is accepted wherever a handle is valid.
// `fn`: the caller.  model_form: flowgnn_set_model_jk_residual, which a GCN engine accepts; on a GIN engine the two calls are one.
static int set_jk_residual(flowgnn_engine* e, const char* fn, bool model_form, int emb_dim, int jk, int residual) {
    const std::string who = std::string(fn) + ": ";
    if (jk != FLOWGNN_JK_LAST && jk != FLOWGNN_JK_SUM)
        return refuse(e, FLOWGNN_ERR_ARG, who + "jk is " + std::to_string(jk) + "; the values are FLOWGNN_JK_LAST (0) and FLOWGNN_JK_SUM (1)");
    if (residual != 0 && residual != 1)
        return refuse(e, FLOWGNN_ERR_ARG, who + "residual is " + std::to_string(residual) + "; the values are 0 (off) and 1 (on)");
    if (int rc = width_argument(e, who, emb_dim)) return rc;
    if (jk != FLOWGNN_JK_LAST || residual) {
        const bool gcn = e->model_id == FLOWGNN_MODEL_GCN;
        if (gcn && !model_form)
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "GCN's rows in HBM are post-linear (W_l a_l + b_l, not h_l), so a residual needs a second row stream through its layer "
                           "kernel: that form does not exist yet (FLOWGNN_MODEL_GIN only) under this call -- it is "
                           "flowgnn_set_model_jk_residual that carries it for FLOWGNN_MODEL_GCN at width 300");
        if (!gcn && e->model_id != FLOWGNN_MODEL_GIN)
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + (model_form ? "JK sum and the residual exist for FLOWGNN_MODEL_GIN and FLOWGNN_MODEL_GCN only (OGB's gin, gin-virtual, gcn "
                                         "and gcn-virtual at width 300)"
                                       : "JK sum and the residual exist for FLOWGNN_MODEL_GIN only (OGB's gin and gin-virtual at width 300)"));
        if (int rc = width_matches(e, who, false, emb_dim, e->emb_dim)) return rc;
        if (emb_dim != FLOWGNN_EMB_DIM_OGB)
            return refuse(e, FLOWGNN_ERR_UNSUPPORTED, who + "only the 300-wide " + (gcn ? "GCN" : "GIN") + " has these instances (the 100-wide graph-resident kernels and the 100-wide per-layer path have "
                           "none): " + (gcn ? "flowgnn_set_model_emb_dim" : "flowgnn_set_emb_dim") + "(e, 300) first");
    }
    ENGINE_TRY(e, use_device(e));
    e->drop_graph();  // a recorded launch sequence is that of the other setting
    e->jk = jk;
    e->residual = residual;
    e->db.jk = jk;  // (launches are stream-ordered: the setting matters to those enqueued after this call)
    e->db.residual = residual;
    return FLOWGNN_OK;
}

extern "C" {

int flowgnn_set_jk_residual(flowgnn_engine* e, int emb_dim, int jk, int residual) {
    if (!e) return FLOWGNN_ERR_ARG;
    return set_jk_residual(e, "flowgnn_set_jk_residual", false, emb_dim, jk, residual);
}

int flowgnn_set_model_jk_residual(flowgnn_engine* e, int emb_dim, int jk, int residual) {
    if (!e) return FLOWGNN_ERR_ARG;
    return set_jk_residual(e, "flowgnn_set_model_jk_residual", true, emb_dim, jk, residual);
}

int flowgnn_jk_residual(const flowgnn_engine* e, int* jk_out, int* residual_out) {
    if (!e) return -1;
    if (jk_out) *jk_out = e->jk;
    if (residual_out) *residual_out = e->residual;
    return (e->jk != FLOWGNN_JK_LAST || e->residual) ? 1 : 0;
}
}  // extern "C"
