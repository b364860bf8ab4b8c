// occ_plan_fill_main.cpp -- occ_plan (rnascan_amd/csrc/pfmscan_occ_plan.hpp) with its two optional arguments, for
// tests/test_occ_plan_fill_cpu.py.  Reads cases from stdin, one per line:
//     m n_unit cells wide cap fill_blk unit_group n_rec len_0 ... len_{n_rec - 1}
// and prints the plan of each on one line:
//     n_u_max need_blk need_grp  n_cuts cuts...
// The record lengths sit in an exact-size heap buffer, so that an overread is seen by the address sanitizer.
#include <cstdio>
#include <memory>

#include "pfmscan_occ_plan.hpp"

int main()
{
    long long m, n_unit, cells, wide, cap, fill_blk, unit_group, n_rec;
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &m, &n_unit, &cells, &wide, &cap, &fill_blk, &unit_group, &n_rec) == 8) {
        std::unique_ptr<int64_t[]> len(new int64_t[(size_t)n_rec]);
        for (long long r = 0; r < n_rec; ++r) {
            long long v;
            if (std::scanf("%lld", &v) != 1) return 2;
            len[(size_t)r] = v;
        }
        const pfmscan::OccPlan p = pfmscan::occ_plan(len.get(), n_rec, (int)m, n_unit, (int)cells, (int)wide, cap, false, fill_blk, unit_group);
        std::printf("%lld %lld %lld  %zu", (long long)p.n_u_max, (long long)p.need_blk, (long long)p.need_grp, p.cuts.size());
        for (int64_t c : p.cuts) std::printf(" %lld", (long long)c);
        std::printf("\n");
    }
    return 0;
}
