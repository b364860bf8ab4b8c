// pfmscan_sites_lib_host.hip -- the host half of the site profiles of a motif LIBRARY (pfmscan_sites_lib.hip): the hit
// list of a library is put into motif-major order, checked and cut into per-motif groups, and the long accumulators the
// device fills (pfmscan_superacc.hpp) are merged, normalised and rounded.  No device code and no HIP call: the file also
// compiles with a plain C++ compiler (tests/c/fuzz_sites_lib.cpp is built with it under the sanitizers).
//
// An accumulator is uint64 [PFMSCAN_SITE_LIMBS][n_words], limb i of weight 2^(32 i), A = sum of limb i * 2^(32 i), value
// A * 2^-1074.  RAW: what a device call leaves (a limb below 2^63).  NORMALISED: every limb but the top one below 2^32.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pfmscan.h"
#include "pfmscan_superacc.hpp"

namespace {

constexpr int LIMBS = PFMSCAN_SITE_LIMBS;

// the record table as pfmscan_site_groups reads it
bool records_ok(const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec)
{
    for (int64_t r = 0; r < n_rec; ++r) {
        if (rec_off[r] < 0 || rec_len[r] < 0 || rec_len[r] > INT64_MAX - rec_off[r]) return false;
        if (r > 0 && rec_off[r] <= rec_off[r - 1] + rec_len[r - 1]) return false;
    }
    return true;
}

// one walk over a motif-major hit list: the groups are counted (out == false) or written down
int64_t walk(const int64_t *hit_pos, const int32_t *hit_motif, int64_t n_hits, int32_t n_motifs, const int64_t *rec_off,
             const int64_t *rec_len, int64_t n_rec, int32_t m, bool out, int64_t *grp_first, int64_t *grp_rec, int64_t *grp_motif)
{
    int64_t g = 0, r = 0, in_group = 0, last_rec = -1;
    for (int64_t h = 0; h < n_hits; ++h) {
        const int64_t p = hit_pos[h];
        const int32_t k = hit_motif[h];
        if (k < 0 || k >= n_motifs) return -1;
        if (h > 0 && k != hit_motif[h - 1]) {                // the next motif: its groups are those of its own list
            if (k < hit_motif[h - 1]) return -1;
            r = 0;
            last_rec = -1;
        } else if (h > 0 && p <= hit_pos[h - 1]) {
            return -1;
        }
        while (r < n_rec && p >= rec_off[r] + rec_len[r]) ++r;
        if (r >= n_rec || p < rec_off[r] || (int64_t)m > rec_off[r] + rec_len[r] - p) return -1;
        if (r != last_rec || in_group == PFMSCAN_SITE_GROUP) {
            if (out) {
                grp_first[g] = h;
                grp_rec[g] = r;
                grp_motif[g] = k;
            }
            ++g;
            in_group = 0;
            last_rec = r;
        }
        ++in_group;
    }
    return g;
}

}  // namespace

extern "C" {

int pfmscan_site_groups_lib(const int64_t *hit_pos, const int32_t *hit_motif, int64_t n_hits, int32_t n_motifs,
                            const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t m, int64_t capacity,
                            int64_t *grp_first, int64_t *grp_rec, int64_t *grp_motif, int64_t *n_grp)
{
    if (n_grp) *n_grp = 0;
    if (!n_grp || n_hits < 0 || n_motifs < 0 || n_rec < 0 || capacity < 0 || m < 1 || m > PFMSCAN_MAX_WIDTH) return PFMSCAN_E_BADARG;
    if ((n_hits > 0 && (!hit_pos || !hit_motif)) || (n_rec > 0 && (!rec_off || !rec_len))) return PFMSCAN_E_BADARG;
    if (!records_ok(rec_off, rec_len, n_rec)) return PFMSCAN_E_BADARG;
    const int64_t need = walk(hit_pos, hit_motif, n_hits, n_motifs, rec_off, rec_len, n_rec, m, false, nullptr, nullptr, nullptr);
    if (need < 0) return PFMSCAN_E_BADARG;
    *n_grp = need;
    if (need > capacity) return PFMSCAN_E_CAPACITY;
    if (!grp_first || (need > 0 && (!grp_rec || !grp_motif))) return PFMSCAN_E_BADARG;
    walk(hit_pos, hit_motif, n_hits, n_motifs, rec_off, rec_len, n_rec, m, true, grp_first, grp_rec, grp_motif);
    grp_first[need] = n_hits;
    return PFMSCAN_OK;
}

int pfmscan_site_order_lib(const int64_t *hit_pos, const int32_t *hit_motif, int64_t n_hits, int32_t n_motifs, int64_t *order)
{
    (void)hit_pos;                                           // the input order is the caller's word; the sort is stable
    if (n_hits < 0 || n_motifs < 0) return PFMSCAN_E_BADARG;
    if (n_hits > 0 && (!hit_motif || !order)) return PFMSCAN_E_BADARG;
    std::vector<int64_t> at((size_t)n_motifs + 1, 0);
    for (int64_t h = 0; h < n_hits; ++h) {
        const int32_t k = hit_motif[h];
        if (k < 0 || k >= n_motifs) return PFMSCAN_E_BADARG;
        ++at[(size_t)k + 1];
    }
    for (int32_t k = 0; k < n_motifs; ++k) at[(size_t)k + 1] += at[(size_t)k];
    for (int64_t h = 0; h < n_hits; ++h) order[at[(size_t)hit_motif[h]]++] = h;
    return PFMSCAN_OK;
}

int pfmscan_site_acc_add(uint64_t *dst, const uint64_t *src, int64_t n_acc, int64_t n_words_per_limb)
{
    if (n_acc < 0 || n_words_per_limb < 0) return PFMSCAN_E_BADARG;
    if (n_acc > 0 && n_words_per_limb > 0 && (!dst || !src)) return PFMSCAN_E_BADARG;
    const size_t n = (size_t)n_words_per_limb;
    for (int64_t k = 0; k < n_acc; ++k) {
        uint64_t *d = dst + (size_t)k * LIMBS * n;
        const uint64_t *s = src + (size_t)k * LIMBS * n;
        for (size_t e = 0; e < n; ++e) {
            uint64_t carry = 0;
            for (int i = 0; i < LIMBS; ++i) {
                const uint64_t a = d[(size_t)i * n + e], b = s[(size_t)i * n + e];
                uint64_t t = a + b;
                bool over = t < a;
                t += carry;
                over = over || t < carry;
                if (i < LIMBS - 1) {
                    // a carry out of 64 bits goes to the next limb as 2^32 (only un-normalised inputs get here)
                    d[(size_t)i * n + e] = t & 0xffffffffu;
                    carry = (t >> 32) + (over ? (uint64_t(1) << 32) : 0);
                } else {
                    if (over) return PFMSCAN_E_BADSHAPE;     // beyond 2^46 values of DBL_MAX
                    d[(size_t)i * n + e] = t;
                }
            }
        }
    }
    return PFMSCAN_OK;
}

int pfmscan_site_acc_round(const uint64_t *acc, int64_t n_acc, int64_t n_cells, double *out)
{
    if (n_acc < 0 || n_cells < 0) return PFMSCAN_E_BADARG;
    if (n_acc > 0 && n_cells > 0 && (!acc || !out)) return PFMSCAN_E_BADARG;
    const size_t n = (size_t)n_cells;
    uint32_t w[LIMBS + 4];                                   // A in 32-bit words: the top limb is two, a raw one's carry a third
    for (int64_t k = 0; k < n_acc; ++k) {
        const uint64_t *a = acc + (size_t)k * LIMBS * n;
        for (size_t e = 0; e < n; ++e) {
            uint64_t carry = 0;
            int top = -1;                                    // the highest non-zero word
            for (int i = 0; i < LIMBS + 4; ++i) {
                const uint64_t limb = i < LIMBS ? a[(size_t)i * n + e] : 0;
                const uint64_t lo = (limb & 0xffffffffu) + (carry & 0xffffffffu);
                w[i] = (uint32_t)lo;
                carry = (limb >> 32) + (carry >> 32) + (lo >> 32);
                if (w[i]) top = i;
            }
            uint64_t bits = 0;
            if (top >= 0) {
                const int hb = top * 32 + 31 - __builtin_clz(w[top]);
                const int shift = hb > 52 ? hb - 52 : 0;     // A >> shift is the 53-bit significand (or all of a small A)
                if (shift + 1 >= 2047) {
                    bits = uint64_t(0x7ff) << 52;
                } else {
                    const int q = shift >> 5, r = shift & 31;
                    uint64_t mant = ((uint64_t)w[q] >> r) | ((uint64_t)w[q + 1] << (32 - r));
                    if (r) mant |= (uint64_t)w[q + 2] << (64 - r);
                    mant &= (uint64_t(1) << 53) - 1;
                    bits = ((uint64_t)shift << 52) + mant;   // bit 52 of mant carries the exponent field from shift to shift + 1
                    if (shift > 0) {
                        const int rb = shift - 1;
                        const bool half = (w[rb >> 5] >> (rb & 31)) & 1u;
                        bool sticky = (w[rb >> 5] & ((1u << (rb & 31)) - 1u)) != 0;
                        for (int i = 0; i < (rb >> 5) && !sticky; ++i) sticky = w[i] != 0;
                        if (half && (sticky || (mant & 1u))) ++bits;      // to nearest, ties to even; past DBL_MAX this is +inf
                    }
                }
            }
            double v;
            std::memcpy(&v, &bits, sizeof(v));
            out[(size_t)k * n + e] = v;
        }
    }
    return PFMSCAN_OK;
}

int pfmscan_site_acc_from_doubles(const double *values, int64_t n, uint64_t *acc_one_cell)
{
    if (n < 0 || n > INT32_MAX || !acc_one_cell || (n > 0 && !values)) return PFMSCAN_E_BADARG;
    for (int i = 0; i < LIMBS; ++i) acc_one_cell[i] = 0;
    for (int64_t h = 0; h < n; ++h) {
        const double v = values[h];
        if (!(v >= 0.0 && v <= 1.7976931348623157e308)) return PFMSCAN_E_BADARG;
        if (v == 0.0) continue;
        uint32_t piece[3];
        const int first = pfmscan::site_acc_pieces(v, piece);
        for (int i = 0; i < 3; ++i)
            if (piece[i]) acc_one_cell[first + i] += piece[i];
    }
    return PFMSCAN_OK;
}

}  // extern "C"
