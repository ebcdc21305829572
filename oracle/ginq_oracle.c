/*
 * ginq_oracle.c -- CPU restatement of FlowGNN's GIN / GIN-VN path in the reference's own number format,
 * ap_fixed<16,6> (Q6.10: 16 bits, 10 fractional, truncate toward -inf, wrap on overflow;
 * GIN/src/dcl.h:58-59 with the ap_fixed defaults AP_TRN / AP_WRAP).  TEST INFRASTRUCTURE (see flowgnn_oracle.h).
 *
 * PINNED to the reference's own sources run in ap_fixed: the kernel sources of GIN/src and GIN-VN/src, compiled against the fixed form of
 * oracle/hls_standin (make -C oracle ref), give the same 16-bit patterns as this file on every input of
 * tests/test_reference_pin_cpu.py, so which statement computes and stores what is no longer a reading.  NOT pinned: the
 * stand-in's ap_fixed is itself written from the published rules (checked against integer formulas, hls_standin/check.cc),
 * not taken from Vitis, and hls::sqrt / hls::recip (load_inputs.cc:130, whose result GIN never uses) follow R3 / R4 of
 * q_oracle.c.  The rules, as the stand-in and this file both have them:
 *   - every arithmetic expression is exact in a wider type; quantisation happens only where a value is stored into
 *     an FM_TYPE / WT_TYPE object: floor to a multiple of 2^-10, then keep the low 16 bits (two's complement);
 *   - a float weight becomes WT_TYPE the same way (host buffers are aligned_vector<WT_TYPE> filled from float,
 *     GIN/src/host.cc:4-12 and host_load.cc);
 *   - ap_fixed / int (finalize.cc:112) has 42 fractional bits before it is stored; storing floors, so the stored
 *     quotient is floor(sum / n) on the 2^-10 grid (the intermediate truncation toward zero at 2^-42 cannot move a
 *     quotient with denominator n <= 500 across a grid point).
 * With those rules every statement of the GIN datapath reduces to integer arithmetic on the 16-bit patterns:
 *     x + y            -> (x + y) mod 2^16                           (load_inputs.cc:207, message_passing.cc:139-145,
 *                                                                     node_embedding.cc:117,133, finalize.cc:78-112)
 *     FM = a * w       -> ((a * w) >> 10) mod 2^16, arithmetic shift  (node_embedding.cc:132)
 *     r += a * w       -> (r + ((a * w) >> 10)) mod 2^16              (node_embedding.cc:180, linear.cc:36-41: r is on
 *                                                                     the grid, so floor(r + p) = r + floor(p))
 *     relu(x)          -> sign bit ? 0 : x                            (util.h:21-25)
 * Sums are therefore independent of their order (arithmetic mod 2^16), which is what lets a batched GPU kernel match
 * this file bit for bit.  Statistics to expect against the float oracle on molhiv-shaped graphs (SURVEY.md section 8c,
 * measured there with the reference sources): Q - float logit mean +0.03, sigma 0.14, max 0.75.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "flowgnn_oracle.h"

#define D 100
#define H 200
#define L 5

typedef int16_t q16;

static const int nd_card[9] = {119, 4, 12, 12, 10, 6, 6, 2, 2};   /* GIN/src/host_load.cc:5 */
static const int ed_card[3] = {5, 6, 2};                          /* :6 */
static const int nd_off[9] = {0, 119, 123, 135, 147, 157, 163, 169, 171}; /* load_inputs.cc:4 */
static const int ed_off[3] = {0, 5, 11};                          /* message_passing.cc:3 */

/* diagnostic: how many stored values left [-32, 32) and wrapped (not thread safe: call with nthreads = 1 to read it) */
static long long g_wraps = 0;
long long orc_ginq_wraps(int reset) { long long v = g_wraps; if (reset) g_wraps = 0; return v; }
static inline q16 wrap16(int32_t x) { if (x < -32768 || x > 32767) g_wraps++; return (q16)(uint16_t)(uint32_t)x; }
static inline q16 q_add(q16 a, q16 b) { return wrap16((int32_t)a + (int32_t)b); }
static inline q16 q_relu(q16 a) { return a < 0 ? 0 : a; }
/* floor(a * w / 1024) on the bit patterns; >> on a negative int32 is an arithmetic shift with gcc (floor) */
static inline int32_t q_mulfloor(q16 a, q16 w) { return ((int32_t)a * (int32_t)w) >> 10; }
q16 orc_q16_from_float(float x)
{
    double f = floor((double)x * 1024.0);
    long long i = (long long)f;
    return (q16)(uint16_t)(uint64_t)i;
}

typedef struct {
    const q16 *nemb, *eemb, *w1, *b1, *w2, *b2, *pw, *pb;
} ginq_w;

static int ginq_one_graph(int n, int e, const int* nf, const int* el, const int* ea, const ginq_w* w, q16* out,
                          q16* h_dump, long n_tot, long node_off)
{
    size_t nn = (size_t)(n > 0 ? n : 1);
    q16* h = (q16*)malloc(sizeof(q16) * nn * D);
    q16* m = (q16*)malloc(sizeof(q16) * nn * D);
    q16 acc[H];
    int rc = 0;
    for (int i = 0; i < e && !rc; i++) {
        int u = el[2 * i], v = el[2 * i + 1];
        if (u < 0 || u >= n || v < 0 || v >= n) rc = 2;
        for (int k = 0; k < 3; k++)
            if (ea[i * 3 + k] < 0 || ea[i * 3 + k] >= ed_card[k]) rc = 3;
    }
    for (int v = 0; v < n && !rc; v++)
        for (int k = 0; k < 9; k++)
            if (nf[v * 9 + k] < 0 || nf[v * 9 + k] >= nd_card[k]) rc = 4;
    if (rc) goto done;

    /* atom encoder, load_inputs.cc:203-209 */
    for (int v = 0; v < n; v++)
        for (int d = 0; d < D; d++) {
            q16 s = 0;
            for (int k = 0; k < 9; k++) s = q_add(s, w->nemb[(nd_off[k] + nf[v * 9 + k]) * D + d]);
            h[v * D + d] = s;
        }
    if (h_dump) memcpy(h_dump + (0 * n_tot + node_off) * D, h, sizeof(q16) * (size_t)n * D);

    for (int l = 0; l < L; l++) {
        /* message passing, message_passing.cc:132-146 (order of the edges is irrelevant mod 2^16) */
        memset(m, 0, sizeof(q16) * nn * D);
        const q16* ee_l = w->eemb + (size_t)l * ORC_ED_FEATURE_PER_LAYER * D;
        for (int i = 0; i < e; i++) {
            int u = el[2 * i], v = el[2 * i + 1];
            for (int d = 0; d < D; d++) {
                q16 edge_embed = 0;
                for (int k = 0; k < 3; k++) edge_embed = q_add(edge_embed, ee_l[(ed_off[k] + ea[i * 3 + k]) * D + d]);
                q16 total = q_add(edge_embed, h[u * D + d]);
                m[v * D + d] = q_add(m[v * D + d], q_relu(total));
            }
        }
        /* node MLP, node_embedding.cc:103-201; eps == 0 (never loaded: globals.cc:3, host.cc:185-200) */
        const q16* w1 = w->w1 + (size_t)l * H * D;
        const q16* b1 = w->b1 + (size_t)l * H;
        const q16* w2 = w->w2 + (size_t)l * D * H;
        const q16* b2 = w->b2 + (size_t)l * D;
        for (int v = 0; v < n; v++) {
            for (int i = 0; i < D; i++) {
                q16 a = q_add(m[v * D + i], h[v * D + i]);                              /* :117 */
                for (int o = 0; o < H; o++) {
                    q16 addend = wrap16(q_mulfloor(a, w1[o * D + i]));                   /* :132 */
                    acc[o] = q_add(addend, i == 0 ? b1[o] : acc[o]);                     /* :133 */
                }
            }
            for (int d = 0; d < D; d++) {
                q16 r = b2[d];
                for (int i = 0; i < H; i++) r = wrap16((int32_t)r + q_mulfloor(q_relu(acc[i]), w2[d * H + i])); /* :180 */
                if (l != L - 1) r = q_relu(r);                                          /* :189 */
                m[v * D + d] = r;
            }
        }
        memcpy(h, m, sizeof(q16) * nn * D);
        if (h_dump) memcpy(h_dump + ((size_t)(l + 1) * n_tot + node_off) * D, h, sizeof(q16) * (size_t)n * D);
    }
    {   /* readout, finalize.cc:36-113 + linear.cc:36-41 */
        q16 res = w->pb[0];
        for (int d = 0; d < D; d++) {
            q16 sum = 0;
            for (int v = 0; v < n; v++) sum = q_add(sum, h[v * D + d]);
            int32_t s = sum, q = s / n;
            if ((s % n != 0) && ((s < 0) != (n < 0))) q--;                              /* floor division */
            q16 hg = wrap16(q);
            res = wrap16((int32_t)res + q_mulfloor(hg, w->pw[d]));
        }
        out[0] = res;
    }
done:
    free(h); free(m);
    return rc;
}

static q16* quantise(const float* src, size_t n)
{
    q16* q = (q16*)malloc(sizeof(q16) * (n ? n : 1));
    for (size_t i = 0; i < n; i++) q[i] = orc_q16_from_float(src[i]);
    return q;
}

/* Same arguments as orc_GIN_compute_graphs (float weights: quantised here as the reference host does);
   out_q receives the 16-bit patterns, out (optional) their value as float = pattern / 1024;
   h_dump (optional) is int16 [6][N_tot][100]. */
int orc_GIN_compute_graphs_q(int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, const int* reload_weights,
                             float* out, int16_t* out_q, const int* node_feature_in, const int* edge_list_in,
                             const int* edge_attr_in, const float* node_embedding_weight_in,
                             const float* edge_embedding_weight_in, const float* node_mlp_1_weights,
                             const float* node_mlp_1_bias, const float* node_mlp_2_weights, const float* node_mlp_2_bias,
                             const float* graph_pred_weights_in, const float* graph_pred_bias_in, int16_t* h_dump,
                             int nthreads)
{
    long* noff = (long*)malloc(sizeof(long) * (size_t)(num_graphs + 1));
    long* eoff = (long*)malloc(sizeof(long) * (size_t)(num_graphs + 1));
    int* widx = (int*)malloc(sizeof(int) * (size_t)(num_graphs + 1));
    int wi = -1, rc = 0, nsets = 0;
    noff[0] = eoff[0] = 0;
    for (int g = 0; g < num_graphs; g++) {
        if (reload_weights[g]) wi++;
        widx[g] = wi;
        noff[g + 1] = noff[g] + nums_of_nodes[g];
        eoff[g + 1] = eoff[g] + nums_of_edges[g];
    }
    nsets = wi + 1;
    long n_tot = noff[num_graphs];
    if (num_graphs > 0 && widx[0] < 0) { free(noff); free(eoff); free(widx); return 1; }
    size_t S = (size_t)(nsets > 0 ? nsets : 1);
    q16* nemb = quantise(node_embedding_weight_in, S * ORC_ND_FEATURE_TOTAL * D);
    q16* eemb = quantise(edge_embedding_weight_in, S * L * ORC_ED_FEATURE_PER_LAYER * D);
    q16* w1 = quantise(node_mlp_1_weights, S * L * H * D);
    q16* b1 = quantise(node_mlp_1_bias, S * L * H);
    q16* w2 = quantise(node_mlp_2_weights, S * L * D * H);
    q16* b2 = quantise(node_mlp_2_bias, S * L * D);
    q16* pw = quantise(graph_pred_weights_in, S * D);
    q16* pb = quantise(graph_pred_bias_in, S);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) num_threads(nthreads > 1 ? nthreads : 1)
#endif
    for (int g = 0; g < num_graphs; g++) {
        int s = widx[g];
        ginq_w w;
        w.nemb = nemb + (size_t)s * ORC_ND_FEATURE_TOTAL * D;
        w.eemb = eemb + (size_t)s * L * ORC_ED_FEATURE_PER_LAYER * D;
        w.w1 = w1 + (size_t)s * L * H * D;
        w.b1 = b1 + (size_t)s * L * H;
        w.w2 = w2 + (size_t)s * L * D * H;
        w.b2 = b2 + (size_t)s * L * D;
        w.pw = pw + (size_t)s * D;
        w.pb = pb + (size_t)s;
        q16 o = 0;
        int r = ginq_one_graph(nums_of_nodes[g], nums_of_edges[g], node_feature_in + noff[g] * 9, edge_list_in + eoff[g] * 2,
                               edge_attr_in + eoff[g] * 3, &w, &o, h_dump, n_tot, noff[g]);
        if (out_q) out_q[g] = o;
        if (out) out[g] = (float)o / 1024.0f;
        if (r) {
#ifdef _OPENMP
#pragma omp critical
#endif
            rc = r;
        }
    }
    free(nemb); free(eemb); free(w1); free(b1); free(w2); free(b2); free(pw); free(pb);
    free(noff); free(eoff); free(widx);
    return rc;
}
