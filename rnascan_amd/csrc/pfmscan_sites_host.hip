// pfmscan_sites_host.hip -- the host half of the site profiles (pfmscan_sites.hip): a sorted hit list is checked against
// the record table and cut into the groups whose sums the device produces.  No device code and no HIP call: the file
// also compiles with a plain C++ compiler (tests/c/fuzz_sites.cpp is built with it under the sanitizers).
//
// A group is at most PFMSCAN_SITE_GROUP consecutive hits of ONE record, counted from that record's first hit: which
// hits share a group depends on the hits of their record alone, never on the batch, the chunk or the rank that holds it.
#include <cstddef>
#include <cstdint>

#include "../../include/pfmscan.h"

extern "C" int pfmscan_site_groups(const int64_t *hit_pos, int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len,
                                   int64_t n_rec, int32_t m, int64_t capacity, int64_t *grp_first, int64_t *grp_rec,
                                   int64_t *n_grp)
{
    if (n_grp) *n_grp = 0;
    if (!n_grp || n_hits < 0 || n_rec < 0 || capacity < 0 || m < 1 || m > PFMSCAN_MAX_WIDTH) return PFMSCAN_E_BADARG;
    if ((n_hits > 0 && !hit_pos) || (n_rec > 0 && (!rec_off || !rec_len))) return PFMSCAN_E_BADARG;
    // the record table, as pfmscan_profile_colsums_host reads it (the stream's length is not known here: a record only
    // has to lie at a position an int64 can hold, behind the record before it and that record's separator)
    for (int64_t r = 0; r < n_rec; ++r) {
        if (rec_off[r] < 0 || rec_len[r] < 0 || rec_len[r] > INT64_MAX - rec_off[r]) return PFMSCAN_E_BADARG;
        if (r > 0 && rec_off[r] <= rec_off[r - 1] + rec_len[r - 1]) return PFMSCAN_E_BADARG;
    }
    // pass 1: every hit lies in a record, behind the hit before it; count the groups
    int64_t need = 0, r = 0, in_group = 0, last_rec = -1;
    for (int64_t h = 0; h < n_hits; ++h) {
        const int64_t p = hit_pos[h];
        if (h > 0 && p <= hit_pos[h - 1]) return PFMSCAN_E_BADARG;
        while (r < n_rec && p >= rec_off[r] + rec_len[r]) ++r;
        if (r >= n_rec || p < rec_off[r] || (int64_t)m > rec_off[r] + rec_len[r] - p) return PFMSCAN_E_BADARG;
        if (r != last_rec || in_group == PFMSCAN_SITE_GROUP) {
            ++need;
            in_group = 0;
            last_rec = r;
        }
        ++in_group;
    }
    *n_grp = need;
    if (need > capacity) return PFMSCAN_E_CAPACITY;
    if (!grp_first || (need > 0 && !grp_rec)) return PFMSCAN_E_BADARG;
    // pass 2: the same walk, written down
    int64_t g = 0;
    r = 0;
    in_group = 0;
    last_rec = -1;
    for (int64_t h = 0; h < n_hits; ++h) {
        const int64_t p = hit_pos[h];
        while (p >= rec_off[r] + rec_len[r]) ++r;
        if (r != last_rec || in_group == PFMSCAN_SITE_GROUP) {
            grp_first[g] = h;
            grp_rec[g] = r;
            ++g;
            in_group = 0;
            last_rec = r;
        }
        ++in_group;
    }
    grp_first[g] = n_hits;
    return PFMSCAN_OK;
}
