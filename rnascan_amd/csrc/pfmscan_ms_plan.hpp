// pfmscan_ms_plan.hpp -- the passes of the multi-site model (pfmscan_multisite.hip): which records and which motifs share the
// scratch planes of one pass.  A pass holds two doubles (the activity, then the forward product and at last the site
// posterior) per position and motif, for the positions from its first record's offset to its last record's end.
// Host only, no HIP: tests/c/ms_plan_main.cpp compiles it alone, under sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace pfmscan {

struct MsPass {
    int64_t r0, r1;              // records [r0, r1)
    int q0, nq;                  // motifs [q0, q0 + nq)
    int64_t base, span;          // stream position p of the pass lies at p - base of a plane of span doubles
};

// rec_off / rec_len: a checked record table (ascending, disjoint).  cap: doubles of scratch a pass may use; a pass of one
// record and one motif is taken whatever it needs.  Records are taken greedily while ONE motif fits, then as many motifs as fit
// beside it.  -> the passes in (records, motifs) order and the doubles of the largest (need).
inline std::vector<MsPass> ms_plan(const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int n_motifs, int64_t cap, int64_t &need)
{
    std::vector<MsPass> out;
    need = 0;
    if (n_motifs <= 0) return out;
    const int64_t half = std::max<int64_t>(cap / 2, 1);           // positions x motifs of a pass
    int64_t r0 = 0;
    while (r0 < n_rec) {
        const int64_t base = rec_off[r0];
        int64_t r1 = r0 + 1, span = rec_len[r0];
        while (r1 < n_rec) {
            const int64_t s = rec_off[r1] - base + rec_len[r1];   // ascending: the end of r1 is the end of the pass
            if (s > half) break;
            span = s;
            ++r1;
        }
        const int64_t fit = span > 0 ? half / span : (int64_t)n_motifs;
        const int nq = (int)std::min<int64_t>(std::max<int64_t>(fit, 1), n_motifs);
        for (int q0 = 0; q0 < n_motifs; q0 += nq) {
            const int n = std::min(nq, n_motifs - q0);
            out.push_back(MsPass{r0, r1, q0, n, base, span});
            need = std::max(need, 2 * span * n);
        }
        r0 = r1;
    }
    return out;
}

}  // namespace pfmscan
