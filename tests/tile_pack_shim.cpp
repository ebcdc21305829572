// C face of flowgnn_amd/csrc/tile_pack.h for tests/test_tile_pack_cpu.py (ctypes).
#include "tile_pack.h"

extern "C" {
void* tp_plan(int rows, int edges, int sub_rows, int sub_edges, int balance, int binpack, int threads, int num_graphs, const int* nn, const int* ne) {
    fg::TileLimits lim;
    lim.rows = rows; lim.edges = edges; lim.sub_rows = sub_rows; lim.sub_edges = sub_edges;
    lim.balance = balance != 0; lim.binpack = binpack != 0; lim.threads = threads;
    fg::TilePlan* p = new fg::TilePlan();
    fg::plan_tiles(lim, num_graphs, nn, ne, p);
    return p;
}
static const std::vector<int>& tp_vec(const void* plan, int which) {
    const fg::TilePlan* p = (const fg::TilePlan*)plan;
    const std::vector<int>* v[] = {&p->row_start, &p->graph_start, &p->bp_list, &p->bp_lrow, &p->bp_graph, &p->bp_row, &p->sub, &p->big_row, &p->big_graph};
    return *v[which];
}
int tp_len(const void* plan, int which) { return (int)tp_vec(plan, which).size(); }
const int* tp_data(const void* plan, int which) { return tp_vec(plan, which).data(); }
int tp_ok(const void* plan) { return ((const fg::TilePlan*)plan)->ok; }
int tp_sub_ok(const void* plan) { return ((const fg::TilePlan*)plan)->sub_ok; }
double tp_fill(const void* plan) { return ((const fg::TilePlan*)plan)->fill; }
double tp_sub_fill(const void* plan) { return ((const fg::TilePlan*)plan)->sub_fill; }
void tp_free(void* plan) { delete (fg::TilePlan*)plan; }
double tp_greedy_fill(int rows, int edges, int num_graphs, const int* nn, const int* ne) { return fg::greedy_tile_fill(rows, edges, num_graphs, nn, ne); }
}
