// pfmscan_fp_plan.hpp -- the tiles of a posterior site map over averaged-structure profiles (pfmscan_footprint_profile.hip):
// how many tiles of `tile` positions every record has, numbered in record order, and whether one launch can hold them.
// Host only, no HIP: tests/c/fp_plan_main.cpp compiles it alone, under sanitizers.
#pragma once
#include <cstdint>
#include <vector>

namespace pfmscan {

constexpr int64_t FP_MAX_TILES = 0x7FFFFFFF;                       // a workgroup per tile: the x dimension of a grid

// tiles[r + 1] = tiles[r] + ceil(len[r] / tile), tiles[0] = 0 (a record without positions has no tile; one shorter than the
// motif still has: its positions are written) -> the tiles of the call, or -1 when they pass FP_MAX_TILES (the prefix then
// stops at the record that passed it; no sum overflows: the test is made before the addition).  tile >= 1, len[r] >= 0.
inline int64_t fp_tile_prefix(const int64_t *rec_len, int64_t n_rec, int64_t tile, std::vector<int64_t> &tiles)
{
    tiles.assign((size_t)n_rec + 1, 0);
    for (int64_t r = 0; r < n_rec; ++r) {
        const int64_t n = rec_len[r] / tile + (rec_len[r] % tile != 0);   // no len + tile - 1: len may be near 2^63
        if (n > FP_MAX_TILES - tiles[r]) return -1;
        tiles[r + 1] = tiles[r] + n;
    }
    return tiles[n_rec];
}

}  // namespace pfmscan
