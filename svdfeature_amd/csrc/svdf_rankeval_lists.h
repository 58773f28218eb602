// svdf_rankeval_lists.h -- the host-only geometry of svdf_rank_eval_positions: the cut of a call into pieces of
// whole sections and the rows and tiles of a piece's sweep.  Plain C++ without a device call: Engine::rank_eval_run launches what these
// functions say, and the test probe svdf_rank_geometry reports it from a host-only handle.
#ifndef SVDF_RANKEVAL_LISTS_H_
#define SVDF_RANKEVAL_LISTS_H_

#include <cstdint>
#include <vector>

namespace svdf {

// The piece that starts at section s0: whole sections while their load -- load(s), the entries section s sends to the device -- stays
// within the budget; always at least one section.  Returns its end.
template <typename Load>
static inline long rank_eval_piece(long s0, long S, int64_t budget, Load load) {
    long s1 = s0;
    int64_t sum = 0;
    while (s1 < S) {
        const int64_t add = load(s1);
        if (s1 > s0 && sum + add > budget) break;
        sum += add;
        s1++;
    }
    return s1;
}

struct RankEvalRows {
    std::vector<int> row_sec, row_first, row_p0, tile_r0;   // [nrow] [nrow] [nrow + 1] [ntile + 1], every index local to the piece
    int nrow() const { return (int)row_sec.size(); }
    int ntile() const { return (int)tile_r0.size() - 1; }
};

// Rows (a section, or a slice of at most tile_pos of its positives; a section without positives has none) and tiles of consecutive rows
// (at most tile_rows of them, at most tile_pos positives) of the piece [s0, s1).
static inline void rank_eval_rows(const int64_t *pos_ptr, long s0, long s1, int tile_rows, int tile_pos, RankEvalRows &out) {
    out.row_sec.clear(); out.row_first.clear(); out.row_p0.clear(); out.tile_r0.clear();
    for (long s = s0; s < s1; s++) {
        const int p0 = (int)(pos_ptr[s] - pos_ptr[s0]), p1 = (int)(pos_ptr[s + 1] - pos_ptr[s0]);
        for (int a = p0; a < p1; a += tile_pos) { out.row_sec.push_back((int)(s - s0)); out.row_first.push_back(a == p0 ? 1 : 0); out.row_p0.push_back(a); }
    }
    out.row_p0.push_back((int)(pos_ptr[s1] - pos_ptr[s0]));
    const int nrow = out.nrow();
    for (int r = 0; r < nrow;) {
        out.tile_r0.push_back(r);
        int e = r + 1;
        while (e < nrow && e - r < tile_rows && out.row_p0[(size_t)e + 1] - out.row_p0[(size_t)r] <= tile_pos) e++;
        r = e;
    }
    out.tile_r0.push_back(nrow);
}

}  // namespace svdf
#endif
