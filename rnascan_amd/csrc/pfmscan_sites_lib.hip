// pfmscan_sites_lib.hip -- site profiles of a motif LIBRARY: the profile rows and the letters under the hits of every motif
// of one width, summed PER MOTIF in one pass (include/pfmscan.h, "site profiles of a library").
//
// The hit list is motif-major; the groups of motif k are the groups of its own hit list (pfmscan_sites_lib_host.hip), and
// a group's cell is computed in the order of k_site_sums (pfmscan_sites.hip; tests/sites_rules.py restates it).  What
// is new is where the group cells go: not home as rows, but into the motif's LONG ACCUMULATOR, the exact integer
// sum of value / 2^-1074 in PFMSCAN_SITE_LIMBS 64-bit limbs per cell (pfmscan_superacc.hpp).  Integer additions commute
// and associate, so the limbs are the same whatever the schedule: the adds are 64-bit integer atomics and the result
// is still a function of the input alone.  No float atomics.
//
//   k_site_check_lib    one lane per group and per hit: the group table is monotone and covers exactly the hits, no group
//                       is empty or longer than PFMSCAN_SITE_GROUP, grp_motif does not descend and lies in [0, n_motifs),
//                       every record lies inside the stream, the positions ascend strictly inside one motif and every
//                       window lies inside the record of its group.
//   k_site_sums_lib<T>  one WAVE per group, four groups per workgroup (library groups are short: at C5 size nearly every
//                       (motif, record) pair holds one hit).  Lane <-> flat cell e = 7 j + c (8 j + k for the counts), 64
//                       cells at a time; four named accumulators per lane for the hits = 0 .. 3 (mod 4) of the group --
//                       the four waves of k_site_sums -- combined as ((a0 + a1) + a2) + a3.  A finite cell > 0 is cut
//                       into three 32-bit pieces and each non-zero piece is added to its limb with one atomicAdd on
//                       unsigned long long; a non-zero count with one.  The validity check rides along as in k_site_sums;
//                       a group cell that overflowed to +inf from finite cells is a key of its own (SITE_OVERFLOW), and
//                       a non-finite cell is never decomposed.  Whatever the tables hold, a load happens only for a row
//                       inside a record that lies inside the stream, and an add only inside the accumulator of a motif
//                       in [0, n_motifs).
//   k_site_verdict      as for one motif (pfmscan_sites.hpp).
//
// No kernel uses scratch, no workgroup waits on another, 64-bit element indices throughout.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "pfmscan_sites.hpp"
#include "pfmscan_superacc.hpp"

using namespace pfmscan;

namespace {

constexpr int LIB_BLOCK = 256;
constexpr int LIB_WAVES = LIB_BLOCK / 64;                    // groups per workgroup
constexpr int LIB_CHECK_BLOCK = 256;
constexpr int64_t SITE_OVERFLOW = INT64_MAX - 1;             // above every element index: a bad input cell wins the minimum
constexpr int LIMBS = PFMSCAN_SITE_LIMBS;

struct SiteLibArgs {
    int64_t n_pos;                                           // rows / codes of the stream buffer
    const int64_t *hit_pos;                                  // [n_hits] motif-major
    int64_t n_hits;
    const int64_t *grp_first, *grp_rec, *grp_motif;          // [n_grp + 1], [n_grp], [n_grp]
    int64_t n_grp;
    const int64_t *rec_off, *rec_len;                        // [n_rec]
    int64_t n_rec;
    int n_motifs, m, flank;
};

template <typename T> struct LibCell { using Acc = double; static constexpr int CS = 7; };
template <> struct LibCell<uint8_t> { using Acc = uint32_t; static constexpr int CS = 8; };

__global__ __launch_bounds__(LIB_CHECK_BLOCK) void k_site_check_lib(SiteLibArgs a, int64_t *__restrict__ blk)
{
    __shared__ int64_t sh[LIB_CHECK_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * LIB_CHECK_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < a.n_grp) {
        const int64_t f = a.grp_first[i], e = a.grp_first[i + 1], r = a.grp_rec[i], k = a.grp_motif[i];
        bad = f < 0 || e <= f || e > a.n_hits || e - f > PFMSCAN_SITE_GROUP || r < 0 || r >= a.n_rec || k < 0 || k >= a.n_motifs;
        bad = bad || (i == 0 && f != 0) || (i == a.n_grp - 1 && e != a.n_hits) || (i > 0 && a.grp_motif[i - 1] > k);
        if (!bad) bad = !site_inside(a.rec_off[r], a.rec_len[r], a.n_pos);
    }
    if (i < a.n_hits) {
        const int64_t p = a.hit_pos[i];
        int64_t lo = 0, hi = a.n_grp;                        // the last group that starts at or before hit i
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.grp_first[mid] <= i) lo = mid + 1;
            else hi = mid;
        }
        const int64_t g = lo - 1;
        if (g < 0) {
            bad = true;
        } else {
            const int64_t f = a.grp_first[g], e = a.grp_first[g + 1], r = a.grp_rec[g];
            if (!(f <= i && i < e) || r < 0 || r >= a.n_rec) {
                bad = true;
            } else {
                const int64_t off = a.rec_off[r], len = a.rec_len[r];
                if (!site_inside(off, len, a.n_pos) || p < off || (int64_t)a.m > off + len - p) bad = true;
                // the hit before: in this group, or the last one of the group before (no group is empty)
                if (i > 0 && p <= a.hit_pos[i - 1] && (i > f || (g > 0 && a.grp_motif[g - 1] == a.grp_motif[g]))) bad = true;
            }
        }
    }
    const int64_t m = site_block_min(bad ? i : SITE_NONE, sh);
    if (threadIdx.x == 0) blk[blockIdx.x] = m;
}

template <typename T>
__global__ __launch_bounds__(LIB_BLOCK) void k_site_sums_lib(SiteLibArgs a, const T *__restrict__ src,
                                                             unsigned long long *__restrict__ out, int64_t *__restrict__ blk)
{
    using Acc = typename LibCell<T>::Acc;
    constexpr int CS = LibCell<T>::CS;
    constexpr bool ROWS = CS == 7;
    __shared__ int64_t sh[LIB_BLOCK];
    const int t = threadIdx.x, lane = t & 63;
    const int v = __builtin_amdgcn_readfirstlane(t >> 6);    // wave-uniform: the group, its tables and its hit positions
    const int64_t g = (int64_t)blockIdx.x * LIB_WAVES + v;
    const int F = a.flank, W = a.m + 2 * F, ncell = W * CS;
    // the group, clamped to what the buffers hold whatever the tables say (k_site_check_lib judges them)
    int64_t first = 0, roff = 0, rend = 0, k = 0;
    int nh = 0;
    if (g < a.n_grp) {
        first = a.grp_first[g];
        int64_t end = a.grp_first[g + 1];
        const int64_t r = a.grp_rec[g];
        k = a.grp_motif[g];
        first = min(max(first, (int64_t)0), a.n_hits);
        end = min(max(end, first), min(a.n_hits, first + PFMSCAN_SITE_GROUP));
        bool ok = r >= 0 && r < a.n_rec && k >= 0 && k < a.n_motifs;
        if (ok) {
            const int64_t off = a.rec_off[r], len = a.rec_len[r];
            ok = site_inside(off, len, a.n_pos);
            roff = off;
            rend = off + (ok ? len : 0);
        }
        nh = ok ? (int)(end - first) : 0;
    }
    int64_t key = SITE_NONE;

    for (int ch = 0; ch * 64 < ncell; ++ch) {
        const int e = ch * 64 + lane;
        const bool live = e < ncell;
        const int j = e / CS, c = e - j * CS;
        // hit h of the group: flat element index of this lane's cell in the buffer (-1: does not count) and the cell
        auto fetch = [&](int h, T &w, int64_t &el) {
            el = -1;
            w = T(0);
            if (h < nh) {
                const int64_t p = a.hit_pos[first + h];
                if (p >= roff && p < rend) {                 // a hit outside its record reads nothing
                    const int64_t x = p - F + j;
                    if (live && x >= roff && x < rend) {
                        el = ROWS ? x * 7 + c : x;
                        w = src[el];
                    }
                }
            }
        };
        auto add = [&](Acc &acc, T w, int64_t el) {
            if (el >= 0) {
                if constexpr (ROWS) {
                    const double x = (double)w;
                    acc += x;
                    if (!(x >= 0.0 && x < INFINITY)) key = min(key, el);
                } else {
                    acc += (min((int)w, 7) == c) ? 1u : 0u;
                }
            }
        };
        Acc a0 = Acc(0), a1 = Acc(0), a2 = Acc(0), a3 = Acc(0);      // hits = 0, 1, 2, 3 (mod 4): the waves of k_site_sums
        for (int h = 0; h < nh; h += 4) {
            T w0, w1, w2, w3;
            int64_t e0, e1, e2, e3;
            fetch(h, w0, e0);
            fetch(h + 1, w1, e1);
            fetch(h + 2, w2, e2);
            fetch(h + 3, w3, e3);
            add(a0, w0, e0);
            add(a1, w1, e1);
            add(a2, w2, e2);
            add(a3, w3, e3);
        }
        if (live && nh > 0) {
            if constexpr (ROWS) {
                const double cell = ((a0 + a1) + a2) + a3;
                if (cell > 0.0 && cell < INFINITY) {
                    uint32_t piece[3];
                    const int limb = site_acc_pieces(cell, piece);
                    unsigned long long *dst = out + ((size_t)k * LIMBS + limb) * ncell + e;
                    if (piece[0]) atomicAdd(dst, (unsigned long long)piece[0]);
                    if (piece[1]) atomicAdd(dst + ncell, (unsigned long long)piece[1]);
                    if (piece[2]) atomicAdd(dst + 2 * (size_t)ncell, (unsigned long long)piece[2]);
                } else if (cell == INFINITY) {
                    key = min(key, SITE_OVERFLOW);           // from finite cells, or an infinite cell whose index is smaller
                }
            } else {
                const uint32_t n = a0 + a1 + a2 + a3;
                if (n) atomicAdd(out + (size_t)k * ncell + e, (unsigned long long)n);
            }
        }
    }
    if constexpr (ROWS) {
        const int64_t m = site_block_min(key, sh);
        if (t == 0) blk[blockIdx.x] = m;
    }
}

int lib_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int dtype, int64_t n_pos, const int64_t *d_hit_pos,
            int64_t n_hits, const int64_t *d_grp_first, const int64_t *d_grp_rec, const int64_t *d_grp_motif, int64_t n_grp,
            const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, int32_t n_motifs, int32_t m, int32_t flank,
            uint64_t *d_acc, uint64_t *d_counts, int64_t *first_bad, hipStream_t st)
{
    const bool rows = d_profile != nullptr, letters = d_codes != nullptr;
    int rc = site_shape(ctx, rows, dtype, m, flank);
    if (rc) return rc;
    if (n_pos < 0 || n_hits < 0 || n_grp < 0 || n_rec < 0 || n_motifs < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: negative size");
    if (!rows && !letters) return fail(ctx, PFMSCAN_E_BADARG, "site sums: neither codes nor a profile");
    if ((rows && !d_acc) || (letters && !d_counts)) return fail(ctx, PFMSCAN_E_BADARG, "site sums: an input without its output buffer");
    if (rows && (reinterpret_cast<uintptr_t>(d_profile) & 7u)) return fail(ctx, PFMSCAN_E_BADSHAPE, "site sums: the profile must be 8-byte aligned");
    if ((n_hits > 0 || n_grp > 0) && (!d_hit_pos || !d_grp_first || !d_grp_rec || !d_grp_motif || !d_rec_off || !d_rec_len))
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int W = m + 2 * flank;
    if (rows) HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, (size_t)n_motifs * LIMBS * W * 7 * sizeof(uint64_t), st));
    if (letters) HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)n_motifs * W * 8 * sizeof(uint64_t), st));
    if (n_hits == 0 && n_grp == 0) return PFMSCAN_OK;
    const int64_t nb_sums = (n_grp + LIB_WAVES - 1) / LIB_WAVES;
    const int64_t nb_check = (std::max(n_hits, n_grp) + LIB_CHECK_BLOCK - 1) / LIB_CHECK_BLOCK;
    if (nb_sums > INT_MAX || nb_check > INT_MAX) return fail(ctx, PFMSCAN_E_BADSHAPE, "site sums: too many groups for one launch");
    const size_t words = (size_t)(nb_sums + nb_check);
    if ((rc = ensure(ctx, ctx->site_blk, (words + 2) * sizeof(int64_t)))) return rc;
    int64_t *blk = static_cast<int64_t *>(ctx->site_blk.p), *blk_check = blk + nb_sums, *d_verdict = blk + words;
    SiteLibArgs a;
    a.n_pos = n_pos;
    a.hit_pos = d_hit_pos;
    a.n_hits = n_hits;
    a.grp_first = d_grp_first;
    a.grp_rec = d_grp_rec;
    a.grp_motif = d_grp_motif;
    a.n_grp = n_grp;
    a.rec_off = d_rec_off;
    a.rec_len = d_rec_len;
    a.n_rec = n_rec;
    a.n_motifs = n_motifs;
    a.m = m;
    a.flank = flank;
    hipLaunchKernelGGL(k_site_check_lib, dim3((unsigned)nb_check), dim3(LIB_CHECK_BLOCK), 0, st, a, blk_check);
    if (rows && n_grp > 0) {
        unsigned long long *acc = reinterpret_cast<unsigned long long *>(d_acc);
        if (dtype == PFMSCAN_PROFILE_F64)
            hipLaunchKernelGGL(k_site_sums_lib<double>, dim3((unsigned)nb_sums), dim3(LIB_BLOCK), 0, st, a,
                               static_cast<const double *>(d_profile), acc, blk);
        else
            hipLaunchKernelGGL(k_site_sums_lib<float>, dim3((unsigned)nb_sums), dim3(LIB_BLOCK), 0, st, a,
                               static_cast<const float *>(d_profile), acc, blk);
    }
    if (letters && n_grp > 0)
        hipLaunchKernelGGL(k_site_sums_lib<uint8_t>, dim3((unsigned)nb_sums), dim3(LIB_BLOCK), 0, st, a, d_codes,
                           reinterpret_cast<unsigned long long *>(d_counts), blk);
    hipLaunchKernelGGL(k_site_verdict, dim3(1), dim3(SITE_VERDICT_BLOCK), 0, st, blk, rows ? nb_sums : 0, blk_check, nb_check, d_verdict);
    HIP_TRY(ctx, hipGetLastError());
    int64_t v[2] = {SITE_NONE, SITE_NONE};
    HIP_TRY(ctx, hipMemcpyAsync(v, d_verdict, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (v[1] != SITE_NONE)
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: the group table does not cover the motif-major hits in order, a motif index "
                                           "descends or is no motif, a hit's window leaves the record of its group, or a record "
                                           "lies outside the stream");
    if (v[0] == SITE_OVERFLOW)
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: the cells of one group overflow to infinity although each is finite");
    return site_verdict(ctx, v, 0, first_bad);
}

}  // namespace

extern "C" {

int pfmscan_site_sums_lib_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                              const int64_t *d_hit_pos, int64_t n_hits, const int64_t *d_grp_first, const int64_t *d_grp_rec,
                              const int64_t *d_grp_motif, int64_t n_grp, const int64_t *d_rec_off, const int64_t *d_rec_len,
                              int64_t n_rec, int32_t n_motifs, int32_t m, int32_t flank, uint64_t *d_acc, uint64_t *d_counts,
                              int64_t *first_bad, void *stream)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    return lib_dev(ctx, d_codes, d_profile, profile_dtype, n_pos, d_hit_pos, n_hits, d_grp_first, d_grp_rec, d_grp_motif, n_grp,
                   d_rec_off, d_rec_len, n_rec, n_motifs, m, flank, d_acc, d_counts, first_bad,
                   stream ? (hipStream_t)stream : ctx->stream);
}

int pfmscan_site_sums_lib_staged(pfmscan_ctx *ctx, int use_codes, int use_profile, const int64_t *hit_pos, const int32_t *hit_motif,
                                 int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t n_motifs,
                                 int32_t m, int32_t flank, uint64_t *acc, uint64_t *counts, int64_t *first_bad)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: no stream is staged");
    if ((use_codes && !ctx->staged_codes) || (use_profile && !ctx->staged_profile))
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: the staged stream lacks the codes or the profile asked for");
    if (!use_codes && !use_profile) return fail(ctx, PFMSCAN_E_BADARG, "site sums: neither codes nor a profile");
    int rc = site_shape(ctx, use_profile != 0, ctx->staged_dtype, m, flank);
    if (rc) return rc;
    if (n_hits < 0 || n_rec < 0 || n_motifs < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: negative size");
    if ((n_hits > 0 && (!hit_pos || !hit_motif)) || (n_rec > 0 && (!rec_off || !rec_len)) || (use_profile && !acc) || (use_codes && !counts))
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL argument");
    const int W = m + 2 * flank;
    const size_t acc_words = (size_t)n_motifs * LIMBS * W * 7, cnt_words = (size_t)n_motifs * W * 8;
    if (n_hits == 0) {
        if (use_profile) std::fill(acc, acc + acc_words, uint64_t(0));
        if (use_codes) std::fill(counts, counts + cnt_words, uint64_t(0));
        return PFMSCAN_OK;
    }
    // (position, motif) order, as the library scans return their hits -> motif-major
    std::vector<int64_t> order((size_t)n_hits), pos((size_t)n_hits);
    std::vector<int32_t> motif((size_t)n_hits);
    if (pfmscan_site_order_lib(hit_pos, hit_motif, n_hits, n_motifs, order.data()))
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: a hit's motif index is no motif of the library");
    for (int64_t h = 0; h < n_hits; ++h) {
        pos[(size_t)h] = hit_pos[order[(size_t)h]];
        motif[(size_t)h] = hit_motif[order[(size_t)h]];
    }
    std::vector<int64_t> gf((size_t)n_hits + 1, 0), gr((size_t)n_hits + 1, 0), gm((size_t)n_hits + 1, 0);
    int64_t ng = 0;
    if (pfmscan_site_groups_lib(pos.data(), motif.data(), n_hits, n_motifs, rec_off, rec_len, n_rec, m, n_hits, gf.data(), gr.data(),
                                gm.data(), &ng))
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: the hits of a motif must ascend strictly and every window [pos, pos + m) must "
                                           "lie inside one record of a record table whose records ascend, each behind the separator "
                                           "of the one before");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // host tables -> ctx->site_tab: hit_pos | grp_first | grp_rec | grp_motif | rec_off | rec_len
    if ((rc = ensure(ctx, ctx->site_tab, (size_t)(n_hits + 3 * ng + 1 + 2 * n_rec) * sizeof(int64_t)))) return rc;
    int64_t *d = static_cast<int64_t *>(ctx->site_tab.p);
    int64_t *d_first = d + n_hits, *d_grec = d_first + ng + 1, *d_gmot = d_grec + ng, *d_off = d_gmot + ng, *d_len = d_off + n_rec;
    if ((rc = upload(ctx, d, pos.data(), (size_t)n_hits * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d_first, gf.data(), (size_t)(ng + 1) * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d_grec, gr.data(), (size_t)ng * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d_gmot, gm.data(), (size_t)ng * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d_off, rec_off, (size_t)n_rec * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d_len, rec_len, (size_t)n_rec * 8, ctx->stream))) return rc;
    if (use_profile && (rc = ensure(ctx, ctx->site_sums, std::max<size_t>(acc_words * 8, 16)))) return rc;
    if (use_codes && (rc = ensure(ctx, ctx->site_counts, std::max<size_t>(cnt_words * 8, 16)))) return rc;
    rc = lib_dev(ctx, use_codes ? static_cast<const uint8_t *>(ctx->codes.p) : nullptr, use_profile ? ctx->profile.p : nullptr,
                 ctx->staged_dtype, ctx->staged_n, d, n_hits, d_first, d_grec, d_gmot, ng, d_off, d_len, n_rec, n_motifs, m, flank,
                 use_profile ? static_cast<uint64_t *>(ctx->site_sums.p) : nullptr,
                 use_codes ? static_cast<uint64_t *>(ctx->site_counts.p) : nullptr, first_bad, ctx->stream);
    if (rc) return rc;
    std::vector<uint64_t> raw(use_profile ? acc_words : 0);
    if (use_profile) HIP_TRY(ctx, hipMemcpyAsync(raw.data(), ctx->site_sums.p, acc_words * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (use_codes) HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->site_counts.p, cnt_words * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (use_profile) {                                       // raw -> normalised
        std::fill(acc, acc + acc_words, uint64_t(0));
        if (pfmscan_site_acc_add(acc, raw.data(), n_motifs, (int64_t)W * 7)) return fail(ctx, PFMSCAN_E_BADSHAPE, "site sums: accumulator overflow");
    }
    return PFMSCAN_OK;
}

}  // extern "C"
