// tile_pack.h -- the graph-tile planner of flowgnn_set_batch: host arithmetic only (no HIP, no engine), so a CPU test can pin it.
#pragma once
#include <vector>

namespace fg {

struct TileLimits {
    int rows = 0, edges = 0;          // Model::graph_tile_limits (rows <= 0: the model has no graph tiles)
    int sub_rows = 0, sub_edges = 0;  // Model::sub_tile_limits (sub_rows <= 0: no half-tile lists)
    bool balance = true;              // option tile_balance
    bool binpack = false;             // Model::wants_packed_tile_lists
    int threads = 1;                  // host threads the bin packing may use (the plan does not depend on it)
};

// What GraphTiles (common.h) describes, as host vectors; an empty vector: that packing was not built.
struct TilePlan {
    bool ok = false;                          // every graph fits a tile (false: nothing below is built)
    std::vector<int> row_start, graph_start;  // [n_tiles + 1]
    double fill = 0.0;                        // of the FULL-size greedy packing, last tile excluded (what greedy_tile_fill returns)
    std::vector<int> bp_list, bp_lrow;        // [num_graphs]
    std::vector<int> bp_graph, bp_row;        // [bp_tiles + 1]
    std::vector<int> sub, big_row, big_graph; // [n_sub][4], [2 n_big], [2 n_big]
    bool sub_ok = false; double sub_fill = 0.0;
};

void plan_tiles(const TileLimits& lim, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges, TilePlan* plan);

// fill of tiles of `rows` rows / `edges` in-edges when the graphs are packed greedily in batch order, without the last tile; 1 for a
// one-tile batch, 0 when a graph exceeds the limits
double greedy_tile_fill(int rows, int edges, int num_graphs, const int* nums_of_nodes, const int* nums_of_edges);

}  // namespace fg
