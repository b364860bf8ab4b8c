// ms_plan_main.cpp -- the pass plan of the multi-site model (rnascan_amd/csrc/pfmscan_ms_plan.hpp) on its own, for
// tests/test_ms_plan_cpu.py.  Reads cases from stdin, one per line:
//     cap n_motifs n_rec off_0 len_0 ... off_{n_rec - 1} len_{n_rec - 1}
// and prints of each on one line:
//     need n_pass  r0 r1 q0 nq base span ...
// The record table sits in exact-size heap buffers, so that an overread is seen by the address sanitizer.
#include <cstdio>
#include <memory>

#include "pfmscan_ms_plan.hpp"

int main()
{
    long long cap, n_motifs, n_rec;
    while (std::scanf("%lld %lld %lld", &cap, &n_motifs, &n_rec) == 3) {
        std::unique_ptr<int64_t[]> off(new int64_t[(size_t)n_rec]), len(new int64_t[(size_t)n_rec]);
        for (long long r = 0; r < n_rec; ++r) {
            long long o, l;
            if (std::scanf("%lld %lld", &o, &l) != 2) return 2;
            off[(size_t)r] = o;
            len[(size_t)r] = l;
        }
        int64_t need = -1;
        const std::vector<pfmscan::MsPass> plan = pfmscan::ms_plan(off.get(), len.get(), n_rec, (int)n_motifs, cap, need);
        std::printf("%lld %zu ", (long long)need, plan.size());
        for (const pfmscan::MsPass &p : plan)
            std::printf(" %lld %lld %d %d %lld %lld", (long long)p.r0, (long long)p.r1, p.q0, p.nq, (long long)p.base, (long long)p.span);
        std::printf("\n");
    }
    return 0;
}
