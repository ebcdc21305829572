// tile_pack.cpp -- the graph-tile planner of flowgnn_set_batch (tile_pack.h).  Plain C++ like h2d_pack.cpp: no device call, so the
// plan of any batch can be computed, and tested, without a GPU.
#include "tile_pack.h"
#include <algorithm>
#include <functional>

namespace fg {

void host_parallel_for(int parts, const std::function<void(int)>& fn);  // h2d_pack.cpp

namespace {
struct Greedy {
    int tiles = 0;           // 0: a graph exceeds the limits
    long long last_row = 0;  // first row of the last tile
    long long rows = 0;      // rows in all
    double fill(int t_rows) const { return tiles > 1 ? (double)last_row / ((double)(tiles - 1) * t_rows) : (tiles ? 1.0 : 0.0); }
};
// THE greedy loop: whole graphs, in batch order, into tiles of at most `cap` rows / `edges` in-edges.  tr / tg (optional): the first
// row / first graph of every tile.
Greedy greedy_pack(int cap, int edges, int num_graphs, const int* nn, const int* ne, std::vector<int>* tr, std::vector<int>* tg) {
    Greedy r;
    if (tr) { tr->assign(1, 0); tg->assign(1, 0); }
    int tiles = 1, cr = 0, ce = 0;
    for (int g = 0; g < num_graphs; g++) {
        const int n = nn[g], m = ne[g];
        if (n > cap || m > edges) return r;
        if (cr + n > cap || ce + m > edges) {
            tiles++;
            r.last_row = r.rows;
            if (tr) { tr->push_back((int)r.rows); tg->push_back(g); }
            cr = 0; ce = 0;
        }
        cr += n; ce += m; r.rows += n;
    }
    r.tiles = tiles;
    return r;
}

// Bin-packed tile lists (GraphTiles::bp_*): best fit, largest graph first, inside windows of 1 024 consecutive graphs.  Bins are kept in
// buckets by the rows they have left, so placing a graph is a scan over at most t_rows buckets, not over the bins.
// (Flat arrays and a bitmap of the non-empty buckets, windows dealt to the pool of host threads: the packing runs inside every
// flowgnn_set_batch -- the drop-in symbols call it per range -- so it must cost microseconds per thousand graphs.)
void bin_pack(const TileLimits& lim, int num_graphs, const int* nn, const int* ne, TilePlan* p) {
    constexpr int kWindow = 1024;
    const int t_rows = lim.rows, t_edges = lim.edges;
    const int n_win = (num_graphs + kWindow - 1) / kWindow;
    std::vector<int>& list = p->bp_list;
    std::vector<int>& lrow = p->bp_lrow;
    list.resize((size_t)num_graphs); lrow.resize((size_t)num_graphs);  // a window's graphs stay inside its span of the list
    std::vector<std::vector<int>> win_cnt((size_t)n_win), win_rows((size_t)n_win);  // per window: graphs / rows of each of its tiles
    int par = std::min(lim.threads, (n_win + 3) / 4);  // (at least four windows per thread)
    if (par < 1) par = 1;
    host_parallel_for(par, [&](int part) {
        std::vector<int> bin_rows, bin_edges, bin_of((size_t)kWindow), bin_cnt, bin_pos;
        std::vector<std::vector<int>> bucket((size_t)t_rows + 1);  // bucket[r]: bins with r rows left
        std::vector<unsigned long long> nonempty(((size_t)t_rows + 64) / 64);
        std::vector<int> order((size_t)kWindow);
        std::vector<int> count((size_t)t_rows + 2);
        for (int wi_ = part; wi_ < n_win; wi_ += par) {
            const int w0 = wi_ * kWindow;
            const int w1 = w0 + kWindow < num_graphs ? w0 + kWindow : num_graphs, wn = w1 - w0;
            // the window's graphs by node count, largest first (counting sort: n <= t_rows; ties in batch order)
            std::fill(count.begin(), count.end(), 0);
            for (int g = w0; g < w1; g++) count[(size_t)(t_rows - nn[g]) + 1]++;
            for (int r = 0; r <= t_rows; r++) count[(size_t)r + 1] += count[(size_t)r];
            for (int g = w0; g < w1; g++) order[(size_t)count[(size_t)(t_rows - nn[g])]++] = g;
            bin_rows.clear();
            bin_edges.clear();
            for (int r = 0; r <= t_rows; r++)
                if (!bucket[(size_t)r].empty()) bucket[(size_t)r].clear();
            std::fill(nonempty.begin(), nonempty.end(), 0ull);
            for (int oi = 0; oi < wn; oi++) {
                const int g = order[(size_t)oi], n = nn[g], m = ne[g];
                int chosen = -1;
                for (int r = n; r <= t_rows && chosen < 0;) {  // the fullest bin that still takes it: the next non-empty bucket from r = n up
                    const size_t wi = (size_t)r >> 6;
                    const unsigned long long bits = nonempty[wi] >> (r & 63);
                    if (!bits) { r = (int)((wi + 1) << 6); continue; }
                    r += __builtin_ctzll(bits);
                    if (r > t_rows) break;
                    std::vector<int>& bk = bucket[(size_t)r];
                    for (size_t k = bk.size(); k-- > 0;)
                        if (bin_edges[(size_t)bk[k]] + m <= t_edges) { chosen = bk[k]; bk[k] = bk.back(); bk.pop_back(); break; }
                    if (chosen >= 0 && bk.empty()) nonempty[wi] &= ~(1ull << (r & 63));
                    r++;
                }
                if (chosen < 0) { chosen = (int)bin_rows.size(); bin_rows.push_back(0); bin_edges.push_back(0); }
                bin_rows[(size_t)chosen] += n;
                bin_edges[(size_t)chosen] += m;
                bin_of[(size_t)oi] = chosen;
                const int left = t_rows - bin_rows[(size_t)chosen];
                bucket[(size_t)left].push_back(chosen);
                nonempty[(size_t)left >> 6] |= 1ull << (left & 63);
            }
            // the window's tiles, in the order the bins were opened; inside a tile the graphs largest first
            const int nb = (int)bin_rows.size();
            bin_cnt.assign((size_t)nb + 1, 0);
            for (int oi = 0; oi < wn; oi++) bin_cnt[(size_t)bin_of[(size_t)oi] + 1]++;
            for (int k = 0; k < nb; k++) bin_cnt[(size_t)k + 1] += bin_cnt[(size_t)k];
            bin_pos.assign(bin_cnt.begin(), bin_cnt.end() - 1);
            std::fill(bin_rows.begin(), bin_rows.end(), 0);  // (reused as the running row inside each tile)
            for (int oi = 0; oi < wn; oi++) {
                const int k = bin_of[(size_t)oi], g = order[(size_t)oi];
                const size_t at = (size_t)w0 + (size_t)bin_pos[(size_t)k]++;
                list[at] = g;
                lrow[at] = bin_rows[(size_t)k];
                bin_rows[(size_t)k] += nn[g];
            }
            win_cnt[(size_t)wi_].resize((size_t)nb);
            win_rows[(size_t)wi_] = bin_rows;
            for (int k = 0; k < nb; k++) win_cnt[(size_t)wi_][(size_t)k] = bin_cnt[(size_t)k + 1] - bin_cnt[(size_t)k];
        }
    });
    p->bp_graph.assign(1, 0);
    p->bp_row.assign(1, 0);
    long long rows_done = 0;
    int graphs_done = 0;
    for (int wi_ = 0; wi_ < n_win; wi_++)
        for (size_t k = 0; k < win_cnt[(size_t)wi_].size(); k++) {
            graphs_done += win_cnt[(size_t)wi_][k];
            rows_done += win_rows[(size_t)wi_][k];
            p->bp_graph.push_back(graphs_done);
            p->bp_row.push_back((int)rows_done);
        }
}

// half-tile runs + the graphs beyond the half-tile limits (GraphTiles::sub / big_*)
void sub_tiles(const TileLimits& lim, int num_graphs, const int* nn, const int* ne, TilePlan* p) {
    const int s_rows = lim.sub_rows, s_edges = lim.sub_edges;
    std::vector<int>& sub = p->sub;
    int cr = 0, ce = 0, g0 = -1, row0 = 0, row = 0;  // the open run: rows, in-edges, first graph, first row; row: first row of graph g
    long long sub_rows_total = 0;
    auto close_run = [&](int g_end) {
        if (g0 >= 0) { sub.push_back(row0); sub.push_back(cr); sub.push_back(g0); sub.push_back(g_end); }
        g0 = -1; cr = 0; ce = 0;
    };
    for (int g = 0; g < num_graphs; row += nn[g], g++) {
        const int n = nn[g], m = ne[g];
        if (n > s_rows || m > s_edges) {  // within the full-tile limits (plan->ok), beyond the half tile: its own full tile
            close_run(g);
            p->big_row.push_back(row); p->big_row.push_back(row + n);
            p->big_graph.push_back(g); p->big_graph.push_back(g + 1);
            continue;
        }
        if (g0 >= 0 && (cr + n > s_rows || ce + m > s_edges)) close_run(g);
        if (g0 < 0) { g0 = g; row0 = row; }
        cr += n; ce += m;
        sub_rows_total += n;
    }
    close_run(num_graphs);
    const size_t n_sub = sub.size() / 4;
    p->sub_ok = true;
    p->sub_fill = n_sub ? (double)sub_rows_total / ((double)n_sub * s_rows) : 0.0;
}
}  // namespace

double greedy_tile_fill(int rows, int edges, int num_graphs, const int* nn, const int* ne) {
    return greedy_pack(rows, edges, num_graphs, nn, ne, nullptr, nullptr).fill(rows);
}

void plan_tiles(const TileLimits& lim, int num_graphs, const int* nn, const int* ne, TilePlan* p) {
    *p = TilePlan{};
    if (lim.rows <= 0 || num_graphs <= 0) return;
    const Greedy full = greedy_pack(lim.rows, lim.edges, num_graphs, nn, ne, &p->row_start, &p->graph_start);
    if (!full.tiles) { p->row_start.clear(); p->graph_start.clear(); return; }
    p->ok = true;
    // how full the tiles are WITHOUT the last one (the tail of the batch, whatever is left over): a shard of a cut job then sees the
    // fill of its graphs' packing, not of its own tail -- a one-tile batch counts as full (one resident launch beats the per-layer
    // sequence on it anyway) -- and takes the path the whole job would take
    p->fill = full.fill(lim.rows);
    // A batch of a few ROUNDS of tiles over the CUs (dataset-sized batches: 4 113 molhiv graphs pack to 410 GIN tiles of 256 rows -- two
    // rounds over 256 CUs, the second 60 % full, at the price of two): the same graphs in tiles of fewer rows, as many tiles as fill
    // whole rounds (512 of ~203 rows), cost each CU two SHORTER tiles.  The smallest row cap whose greedy packing needs no more than
    // rounds x 256 tiles, by bisection; the fill the models' thresholds see stays that of the full-size packing (it describes the
    // graphs, not this choice).
    constexpr int kCUs = 256, kMaxRounds = 8;
    const int rounds = (full.tiles + kCUs - 1) / kCUs, target = rounds * kCUs;
    if (lim.balance && full.tiles > 1 && rounds <= kMaxRounds && full.tiles < target) {
        auto fits_target = [&](int cap) {
            const int t = greedy_pack(cap, lim.edges, num_graphs, nn, ne, nullptr, nullptr).tiles;
            return t > 0 && t <= target;
        };
        int lo = *std::max_element(nn, nn + num_graphs), hi = lim.rows;  // fits_target(hi) holds; find the smallest cap that still does
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            if (fits_target(mid)) hi = mid; else lo = mid + 1;
        }
        if (hi < lim.rows) greedy_pack(hi, lim.edges, num_graphs, nn, ne, &p->row_start, &p->graph_start);
    }
    p->row_start.push_back((int)full.rows);
    p->graph_start.push_back(num_graphs);
    if (lim.binpack && num_graphs > 1) bin_pack(lim, num_graphs, nn, ne, p);
    if (lim.sub_rows > 0) sub_tiles(lim, num_graphs, nn, ne, p);
}

}  // namespace fg
