// occ_plan_main.cpp -- the pass planner of the occupancy family (rnascan_amd/csrc/pfmscan_occ_plan.hpp) on its own, for
// tests/test_occ_plan_cpu.py.  Reads cases from stdin, one per line:
//     m n_unit cells wide cap runs n_rec len_0 ... len_{n_rec - 1}
// and prints the plan of each on one line:
//     n_u_max need_blk need_grp need_run  n_cuts cuts...  n_start start...
// The record lengths sit in an exact-size heap buffer, so that an overread is seen by the address sanitizer.
#include <cstdio>
#include <memory>

#include "pfmscan_occ_plan.hpp"

int main()
{
    long long m, n_unit, cells, wide, cap, runs, n_rec;
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld", &m, &n_unit, &cells, &wide, &cap, &runs, &n_rec) == 7) {
        std::unique_ptr<int64_t[]> len(new int64_t[(size_t)n_rec]);
        for (long long r = 0; r < n_rec; ++r) {
            long long v;
            if (std::scanf("%lld", &v) != 1) return 2;
            len[(size_t)r] = v;
        }
        const pfmscan::OccPlan p = pfmscan::occ_plan(len.get(), n_rec, (int)m, n_unit, (int)cells, (int)wide, cap, runs != 0);
        if (p.blk() != p.start.data() || p.grp() != p.blk() + n_rec + 1 || p.run() != p.grp() + n_rec + 1 || p.n_pass() + 1 != p.cuts.size()) return 3;
        std::printf("%lld %lld %lld %lld  %zu", (long long)p.n_u_max, (long long)p.need_blk, (long long)p.need_grp, (long long)p.need_run, p.cuts.size());
        for (int64_t c : p.cuts) std::printf(" %lld", (long long)c);
        std::printf("  %zu", p.start.size());
        for (int64_t s : p.start) std::printf(" %lld", (long long)s);
        std::printf("\n");
    }
    return 0;
}
