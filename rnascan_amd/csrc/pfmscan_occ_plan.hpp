// pfmscan_occ_plan.hpp -- the pass plan of the occupancy and the expected counts: the prefix tables that number the blocks,
// groups and runs of the records, and how the records and the units (motifs, cells or matrix rows) are cut into passes whose
// block sums fit the scratch cap.  Host only, no HIP: tests/c/occ_plan_main.cpp compiles it alone, under sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace pfmscan {

constexpr int OCC_FANIN = 32;                                      // windows of a block, blocks of a group
constexpr int OCCP_RUN = 8;                                        // blocks of a run (a workgroup of the profile kernels)

struct OccPlan {
    int64_t n_rec = 0;
    bool runs = false;
    std::vector<int64_t> start;   // as uploaded: blk [n_rec + 1], grp [n_rec + 1], then run [n_rec + 1] when runs are numbered
    std::vector<int64_t> cuts;    // pass i holds the records cuts[i] .. cuts[i + 1]
    int64_t n_u_max = 0;          // units of a pass
    int64_t need_blk = 0, need_grp = 0, need_run = 0;   // the most blocks, groups and runs of a pass
    const int64_t *blk() const { return start.data(); }            // prefix of ceil(n_win / 32)
    const int64_t *grp() const { return blk() + n_rec + 1; }       // prefix of ceil(blocks / 32)
    const int64_t *run() const { return grp() + n_rec + 1; }       // prefix of ceil(blocks / OCCP_RUN)
    size_t n_pass() const { return cuts.size() - 1; }
};

// n_unit units of `cells` scratch doubles per block each, under a cap of `cap` doubles: all units in a pass unless the longest
// record's block sums alone pass the cap; then the records are cut greedily -- a pass takes the next record while it has fewer
// than rec_cap records (2^30 columns of the widest matrix, `wide` per unit) and its blocks stay within blk_cap, and always
// holds at least one record.  n_unit, cells, wide and cap are at least 1 (a call without motifs returns before it plans);
// the block sums of the largest pass are need_blk * n_u_max * cells doubles.
// fill_blk > 1: a pass should hold that many blocks (or all the call has) so that level 0 fills the device, so the units of a
// pass are those that leave room for them, not for the longest record alone -- more passes over the units, fewer and larger
// ones over the records; unit_group: a pass that holds a whole group of units holds whole groups only (the matrix rows of a
// pair: a pair cut in two has its weights made twice).  The results do not depend on either.
inline OccPlan occ_plan(const int64_t *rec_len, int64_t n_rec, int m, int64_t n_unit, int cells, int wide, int64_t cap, bool runs,
                        int64_t fill_blk = 1, int64_t unit_group = 1)
{
    OccPlan p;
    p.n_rec = n_rec;
    p.runs = runs;
    p.start.assign((runs ? 3 : 2) * (size_t)(n_rec + 1), 0);
    int64_t *blk = p.start.data(), *grp = blk + n_rec + 1, *run = grp + n_rec + 1;
    int64_t max_blk = 0;
    for (int64_t r = 0; r < n_rec; ++r) {
        const int64_t nw = std::max<int64_t>(rec_len[r] - m + 1, 0), nb = (nw + OCC_FANIN - 1) / OCC_FANIN;
        blk[r + 1] = blk[r] + nb;
        grp[r + 1] = grp[r] + (nb + OCC_FANIN - 1) / OCC_FANIN;
        if (runs) run[r + 1] = run[r] + (nb + OCCP_RUN - 1) / OCCP_RUN;
        max_blk = std::max(max_blk, nb);
    }
    const int64_t room_blk = std::max<int64_t>({max_blk, std::min(fill_blk, blk[n_rec]), 1});
    p.n_u_max = std::min<int64_t>(n_unit, std::max<int64_t>(1, cap / (room_blk * cells)));
    if (p.n_u_max > unit_group) p.n_u_max -= p.n_u_max % unit_group;
    const int64_t blk_cap = std::max<int64_t>(cap / (p.n_u_max * cells), 1);
    const int64_t rec_cap = std::max<int64_t>((int64_t(1) << 30) / (p.n_u_max * wide), 1);
    p.cuts.assign(1, 0);
    for (int64_t r0 = 0; r0 < n_rec;) {
        int64_t r1 = r0 + 1;
        while (r1 < n_rec && r1 - r0 < rec_cap && blk[r1 + 1] - blk[r0] <= blk_cap) ++r1;
        p.cuts.push_back(r1);
        p.need_blk = std::max(p.need_blk, blk[r1] - blk[r0]);
        p.need_grp = std::max(p.need_grp, grp[r1] - grp[r0]);
        if (runs) p.need_run = std::max(p.need_run, run[r1] - run[r0]);
        r0 = r1;
    }
    return p;
}

}  // namespace pfmscan
