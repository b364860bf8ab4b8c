// fp_plan_main.cpp -- the tile prefix of the posterior site map on profiles (rnascan_amd/csrc/pfmscan_fp_plan.hpp) on its own,
// for tests/test_fp_plan_cpu.py.  Reads cases from stdin, one per line:
//     tile n_rec len_0 ... len_{n_rec - 1}
// and prints of each on one line:
//     n_tiles  n_prefix prefix...
// The record lengths sit in an exact-size heap buffer, so that an overread is seen by the address sanitizer.
#include <cstdio>
#include <memory>

#include "pfmscan_fp_plan.hpp"

int main()
{
    long long tile, n_rec;
    while (std::scanf("%lld %lld", &tile, &n_rec) == 2) {
        std::unique_ptr<int64_t[]> len(new int64_t[(size_t)n_rec]);
        for (long long r = 0; r < n_rec; ++r) {
            long long v;
            if (std::scanf("%lld", &v) != 1) return 2;
            len[(size_t)r] = v;
        }
        std::vector<int64_t> tiles;
        const int64_t n = pfmscan::fp_tile_prefix(len.get(), n_rec, tile, tiles);
        if (tiles.size() != (size_t)n_rec + 1 || tiles[0] != 0) return 3;
        std::printf("%lld  %zu", (long long)n, tiles.size());
        for (int64_t t : tiles) std::printf(" %lld", (long long)t);
        std::printf("\n");
    }
    return 0;
}
