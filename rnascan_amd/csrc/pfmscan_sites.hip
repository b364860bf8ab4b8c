// pfmscan_sites.hip -- site profiles: the profile rows and the letters under aligned hit windows, summed per group of
// hits.  What the sites of a motif look like (the structural context under them, the meta-profile over their flanks),
// and what a structure PFM is made from: average_structure.py:28-42 counts the aligned context letters and
// pfmutil.py:136-151 normalises per position; summing the rows under the hit windows is the same operation on hits.
//
// Hit h of width m with flank F covers the W = m + 2 F columns j of stream rows x = pos[h] - F + j; a column COUNTS only
// when x lies inside the hit's record (flanks that hang over a record end are skipped, not read).  The hits of a record
// are cut into groups of at most PFMSCAN_SITE_GROUP, anchored at the record's first hit (pfmscan_sites_host.hip), and
// the device produces PER-GROUP cells: double sums[W][7] of the rows, uint32 counts[W][8] of the codes.  The host adds
// the groups up with math.fsum, which is exactly rounded, so the result has the same bits however the hits were cut into
// batches, chunks or ranks.  Inside a group the order of ADDITIONS is a function of the group alone:
//
//       wave v of 4   acc = 0.0 per cell; hits v, v + 4, v + 8, ... of the group in ascending order: acc += (double) cell
//                     for the hits whose column counts (only additions, fp32 rows widened first)
//       group         ((wave 0 + wave 1) + wave 2) + wave 3
//
//     tests/sites_rules.py restates this in numpy; the kernels equal it bit for bit.
//
//   k_site_check    one lane per group and per hit: the group table is monotone, covers exactly the hits, no group is
//                   longer than PFMSCAN_SITE_GROUP, every record lies inside the stream, every hit lies behind the hit
//                   before it and its window inside the record of its group.
//   k_site_sums<T>  one workgroup per group.  Lane <-> flat cell e = 7 j + c (8 j + k for the counts), 64 cells per wave
//                   at a time: for one hit a wave reads the 64 consecutive elements from (pos - F) * 7 + 64 * chunk, one
//                   coalesced 256 / 512 bytes (codes: 8 lanes share a byte).  The hit position is wave-uniform and read
//                   once per wave.  One accumulator per lane; the hits are walked again for the next 64 cells.  The
//                   cells of the next SITE_AHEAD hits of the wave are in flight while the current ones are added.  The
//                   validity check (finite, >= 0) rides along: the smallest bad flat element index per workgroup.
//                   Whatever the tables hold, a load happens only for a row inside a record that lies inside the stream.
//   k_site_verdict  one workgroup: the smallest key of either kind.
//
// No global atomics, no workgroup waits on another, 64-bit element indices throughout.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "pfmscan_sites.hpp"

using namespace pfmscan;

namespace {

constexpr int SITE_BLOCK = 256;
constexpr int SITE_WAVES = SITE_BLOCK / 64;
constexpr int SITE_AHEAD = 4;                    // hits of a wave whose cells are loaded together
constexpr int SITE_CHECK_BLOCK = 256;

struct SiteArgs {
    int64_t n_pos;                               // rows / codes of the stream buffer
    const int64_t *hit_pos;                      // [n_hits] stream positions (of the WHOLE stream: row_base is subtracted)
    int64_t n_hits;
    const int64_t *grp_first, *grp_rec;          // [n_grp + 1], [n_grp]: indices into hit_pos, into the record table
    int64_t n_grp;
    const int64_t *rec_off, *rec_len;            // [n_rec]; row of a record in the buffer = rec_off[r] - row_base
    int64_t n_rec, row_base;
    int64_t hit_lo, hit_hi;                      // the hits these groups must cover exactly
    int m, flank;
};

template <typename T> struct SiteCell { using Acc = double; static constexpr int CS = 7; };
template <> struct SiteCell<uint8_t> { using Acc = uint32_t; static constexpr int CS = 8; };

__global__ __launch_bounds__(SITE_CHECK_BLOCK) void k_site_check(SiteArgs a, int64_t *__restrict__ blk)
{
    __shared__ int64_t sh[SITE_CHECK_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * SITE_CHECK_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < a.n_grp) {
        const int64_t f = a.grp_first[i], e = a.grp_first[i + 1], r = a.grp_rec[i];
        bad = f < a.hit_lo || e < f || e > a.hit_hi || e - f > PFMSCAN_SITE_GROUP || r < 0 || r >= a.n_rec;
        bad = bad || (i == 0 && f != a.hit_lo) || (i == a.n_grp - 1 && e != a.hit_hi);
        if (!bad) {
            const int64_t off = a.rec_off[r], len = a.rec_len[r];
            bad = off < a.row_base || !site_inside(off - a.row_base, len, a.n_pos);
        }
    }
    if (i < a.hit_hi - a.hit_lo) {
        const int64_t h = a.hit_lo + i, p = a.hit_pos[h];
        if (h > a.hit_lo && p <= a.hit_pos[h - 1]) bad = true;
        int64_t lo = 0, hi = a.n_grp;                        // the last group that starts at or before h
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.grp_first[mid] <= h) lo = mid + 1;
            else hi = mid;
        }
        const int64_t g = lo - 1;
        if (g < 0) {
            bad = true;
        } else {
            const int64_t f = a.grp_first[g], e = a.grp_first[g + 1], r = a.grp_rec[g];
            if (!(f <= h && h < e) || r < 0 || r >= a.n_rec) {
                bad = true;
            } else {
                const int64_t off = a.rec_off[r], len = a.rec_len[r];
                if (off < a.row_base || !site_inside(off - a.row_base, len, a.n_pos) || p < off || (int64_t)a.m > off + len - p)
                    bad = true;
            }
        }
    }
    const int64_t m = site_block_min(bad ? i : SITE_NONE, sh);
    if (threadIdx.x == 0) blk[blockIdx.x] = m;
}

template <typename T>
__global__ __launch_bounds__(SITE_BLOCK) void k_site_sums(SiteArgs a, const T *__restrict__ src,
                                                          typename SiteCell<T>::Acc *__restrict__ out, int64_t *__restrict__ blk)
{
    using Acc = typename SiteCell<T>::Acc;
    constexpr int CS = SiteCell<T>::CS;
    constexpr bool ROWS = CS == 7;
    __shared__ Acc wsum[SITE_WAVES][64];
    __shared__ int64_t sh[SITE_BLOCK];
    const int t = threadIdx.x, lane = t & 63;
    const int v = __builtin_amdgcn_readfirstlane(t >> 6);    // wave-uniform: the hit positions are read once per wave
    const int64_t g = blockIdx.x;
    const int F = a.flank, W = a.m + 2 * F, ncell = W * CS;
    // the group, clamped to what the buffers hold whatever the tables say (k_site_check judges them)
    int64_t first = a.grp_first[g], end = a.grp_first[g + 1];
    const int64_t r = a.grp_rec[g];
    first = min(max(first, a.hit_lo), a.hit_hi);
    end = min(max(end, first), min(a.hit_hi, first + PFMSCAN_SITE_GROUP));
    int64_t roff = 0, rend = 0;                              // the record's rows, as stream positions
    bool ok = r >= 0 && r < a.n_rec;
    if (ok) {
        const int64_t off = a.rec_off[r], len = a.rec_len[r];
        ok = off >= a.row_base && site_inside(off - a.row_base, len, a.n_pos);
        roff = off;
        rend = off + (ok ? len : 0);
    }
    const int nh = ok ? (int)(end - first) : 0;
    int64_t key = SITE_NONE;

    for (int ch = 0; ch * 64 < ncell; ++ch) {
        const int e = ch * 64 + lane;
        const bool live = e < ncell;
        const int j = e / CS, c = e - j * CS;
        T val[SITE_AHEAD], nxt[SITE_AHEAD];
        int64_t at[SITE_AHEAD], nat[SITE_AHEAD];             // flat element index of a slot's cell in the buffer, -1: does not count
        // slots u = 0 .. SITE_AHEAD - 1 hold hits h0 + 4 u of this wave
        auto fetch = [&](int h0, T (&w)[SITE_AHEAD], int64_t (&el)[SITE_AHEAD]) {
#pragma unroll
            for (int u = 0; u < SITE_AHEAD; ++u) {
                const int h = h0 + SITE_WAVES * u;
                el[u] = -1;
                w[u] = T(0);
                if (h < nh) {
                    const int64_t p = a.hit_pos[first + h];
                    if (p >= roff && p < rend) {             // a hit outside its record reads nothing
                        const int64_t x = p - F + j;
                        if (live && x >= roff && x < rend) {
                            el[u] = ROWS ? (x - a.row_base) * 7 + c : x - a.row_base;
                            w[u] = src[el[u]];
                        }
                    }
                }
            }
        };
        Acc acc = Acc(0);
        fetch(v, val, at);
        for (int h0 = v; h0 < nh; h0 += SITE_WAVES * SITE_AHEAD) {
            const int hn = h0 + SITE_WAVES * SITE_AHEAD;
            if (hn < nh) fetch(hn, nxt, nat);
#pragma unroll
            for (int u = 0; u < SITE_AHEAD; ++u) {
                if (at[u] >= 0) {
                    if constexpr (ROWS) {
                        const double x = (double)val[u];
                        acc += x;
                        if (!(x >= 0.0 && x < INFINITY)) key = min(key, at[u]);
                    } else {
                        acc += (min((int)val[u], 7) == c) ? 1u : 0u;
                    }
                }
            }
            if (hn < nh) {
#pragma unroll
                for (int u = 0; u < SITE_AHEAD; ++u) {
                    val[u] = nxt[u];
                    at[u] = nat[u];
                }
            }
        }
        wsum[t >> 6][lane] = acc;
        __syncthreads();
        if (t < 64 && live) out[g * ncell + e] = ((wsum[0][t] + wsum[1][t]) + wsum[2][t]) + wsum[3][t];
        __syncthreads();
    }
    if constexpr (ROWS) {
        const int64_t m = site_block_min(key, sh);
        if (t == 0) blk[g] = m;
    }
}

int64_t site_check_blocks(int64_t n_hits, int64_t n_grp) { return (std::max(n_hits, n_grp) + SITE_CHECK_BLOCK - 1) / SITE_CHECK_BLOCK; }
// int64 words of scratch one launch set needs: a key per group, a key per check workgroup
size_t site_blk_words(int64_t n_hits, int64_t n_grp) { return (size_t)(n_grp + site_check_blocks(n_hits, n_grp)); }

// Launches of one set of groups on `st`: a.grp_first / a.grp_rec are the set's n_grp groups, which cover hits
// [a.hit_lo, a.hit_hi); sums / counts of group 0 of the set go to d_sums / d_counts; the verdict to d_verdict[0..1].
// blk: scratch of site_blk_words(a.hit_hi - a.hit_lo, a.n_grp).  Asynchronous.
int site_launch(pfmscan_ctx *ctx, const SiteArgs &a, const uint8_t *d_codes, const void *d_profile, int dtype, double *d_sums,
                uint32_t *d_counts, int64_t *blk, int64_t *d_verdict, hipStream_t st)
{
    const int64_t nb_check = site_check_blocks(a.hit_hi - a.hit_lo, a.n_grp);
    if (a.n_grp > INT_MAX || nb_check > INT_MAX) return fail(ctx, PFMSCAN_E_BADSHAPE, "site sums: too many groups for one launch");
    int64_t *blk_check = blk + a.n_grp;
    hipLaunchKernelGGL(k_site_check, dim3((unsigned)nb_check), dim3(SITE_CHECK_BLOCK), 0, st, a, blk_check);
    const bool rows = d_profile && d_sums;
    if (rows && a.n_grp > 0) {
        if (dtype == PFMSCAN_PROFILE_F64)
            hipLaunchKernelGGL(k_site_sums<double>, dim3((unsigned)a.n_grp), dim3(SITE_BLOCK), 0, st, a,
                               static_cast<const double *>(d_profile), d_sums, blk);
        else
            hipLaunchKernelGGL(k_site_sums<float>, dim3((unsigned)a.n_grp), dim3(SITE_BLOCK), 0, st, a,
                               static_cast<const float *>(d_profile), d_sums, blk);
    }
    if (d_codes && d_counts && a.n_grp > 0)
        hipLaunchKernelGGL(k_site_sums<uint8_t>, dim3((unsigned)a.n_grp), dim3(SITE_BLOCK), 0, st, a, d_codes, d_counts, blk);
    hipLaunchKernelGGL(k_site_verdict, dim3(1), dim3(SITE_VERDICT_BLOCK), 0, st, blk, rows ? a.n_grp : 0, blk_check, nb_check,
                       d_verdict);
    HIP_TRY(ctx, hipGetLastError());
    return PFMSCAN_OK;
}

int site_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int dtype, int64_t n_pos, const int64_t *d_hit_pos,
             int64_t n_hits, const int64_t *d_grp_first, const int64_t *d_grp_rec, int64_t n_grp, const int64_t *d_rec_off,
             const int64_t *d_rec_len, int64_t n_rec, int32_t m, int32_t flank, double *d_sums, uint32_t *d_counts,
             int64_t *first_bad, hipStream_t st)
{
    const bool rows = d_profile != nullptr, letters = d_codes != nullptr;
    int rc = site_shape(ctx, rows, dtype, m, flank);
    if (rc) return rc;
    if (n_pos < 0 || n_hits < 0 || n_grp < 0 || n_rec < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: negative size");
    if (!rows && !letters) return fail(ctx, PFMSCAN_E_BADARG, "site sums: neither codes nor a profile");
    if ((rows && !d_sums) || (letters && !d_counts)) return fail(ctx, PFMSCAN_E_BADARG, "site sums: an input without its output buffer");
    if (n_hits == 0 && n_grp == 0) return PFMSCAN_OK;
    if (!d_hit_pos || !d_grp_first || !d_grp_rec || !d_rec_off || !d_rec_len) return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL buffer");
    if (rows && (reinterpret_cast<uintptr_t>(d_profile) & 7u)) return fail(ctx, PFMSCAN_E_BADSHAPE, "site sums: the profile must be 8-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t words = site_blk_words(n_hits, n_grp);
    if ((rc = ensure(ctx, ctx->site_blk, (words + 2) * sizeof(int64_t)))) return rc;
    int64_t *blk = static_cast<int64_t *>(ctx->site_blk.p);
    SiteArgs a;
    a.n_pos = n_pos;
    a.hit_pos = d_hit_pos;
    a.n_hits = n_hits;
    a.grp_first = d_grp_first;
    a.grp_rec = d_grp_rec;
    a.n_grp = n_grp;
    a.rec_off = d_rec_off;
    a.rec_len = d_rec_len;
    a.n_rec = n_rec;
    a.row_base = 0;
    a.hit_lo = 0;
    a.hit_hi = n_hits;
    a.m = m;
    a.flank = flank;
    if ((rc = site_launch(ctx, a, d_codes, d_profile, dtype, d_sums, d_counts, blk, blk + words, st))) return rc;
    int64_t v[2] = {SITE_NONE, SITE_NONE};
    HIP_TRY(ctx, hipMemcpyAsync(v, blk + words, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return site_verdict(ctx, v, 0, first_bad);
}

// the groups of a host hit list (pfmscan_site_groups) against the caller's capacity
int site_cut(pfmscan_ctx *ctx, const int64_t *hit_pos, int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len,
             int64_t n_rec, int32_t m, int64_t capacity, std::vector<int64_t> &grp_first, std::vector<int64_t> &grp_rec,
             int64_t *n_grp)
{
    grp_first.assign((size_t)n_hits + 1, 0);
    grp_rec.assign((size_t)n_hits + 1, 0);
    int64_t n = 0;
    const int rc = pfmscan_site_groups(hit_pos, n_hits, rec_off, rec_len, n_rec, m, n_hits, grp_first.data(), grp_rec.data(), &n);
    if (rc) return fail(ctx, rc, "site sums: the hits must ascend strictly and every window [pos, pos + m) must lie inside one "
                                 "record of a record table whose records ascend, each behind the separator of the one before");
    *n_grp = n;
    if (n > capacity) return fail(ctx, PFMSCAN_E_CAPACITY, "site sums: " + std::to_string(n) + " groups, room for fewer");
    grp_first.resize((size_t)n + 1);
    grp_rec.resize((size_t)n);
    return PFMSCAN_OK;
}

// host tables -> ctx->site_tab on the ctx's stream: hit_pos | grp_first | grp_rec | rec_off | rec_len
int site_upload_tables(pfmscan_ctx *ctx, const int64_t *hit_pos, int64_t n_hits, const std::vector<int64_t> &grp_first,
                       const std::vector<int64_t> &grp_rec, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                       const int64_t **d_hit, const int64_t **d_first, const int64_t **d_grec, const int64_t **d_off,
                       const int64_t **d_len)
{
    const int64_t n_grp = (int64_t)grp_rec.size();
    int rc = ensure(ctx, ctx->site_tab, (size_t)(n_hits + 2 * n_grp + 1 + 2 * n_rec) * sizeof(int64_t));
    if (rc) return rc;
    int64_t *d = static_cast<int64_t *>(ctx->site_tab.p);
    *d_hit = d;
    *d_first = d + n_hits;
    *d_grec = *d_first + n_grp + 1;
    *d_off = *d_grec + n_grp;
    *d_len = *d_off + n_rec;
    if ((rc = upload(ctx, d, hit_pos, (size_t)n_hits * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d + n_hits, grp_first.data(), (size_t)(n_grp + 1) * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d + n_hits + n_grp + 1, grp_rec.data(), (size_t)n_grp * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d + n_hits + 2 * n_grp + 1, rec_off, (size_t)n_rec * 8, ctx->stream))) return rc;
    return upload(ctx, d + n_hits + 2 * n_grp + 1 + n_rec, rec_len, (size_t)n_rec * 8, ctx->stream);
}

}  // namespace

int pfmscan::site_shape(pfmscan_ctx *ctx, bool rows, int dtype, int32_t m, int32_t flank)
{
    if (rows && dtype != PFMSCAN_PROFILE_F32 && dtype != PFMSCAN_PROFILE_F64)
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: profile_dtype must be PFMSCAN_PROFILE_F32 or F64");
    if (m < 1 || flank < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: the width must be at least 1 and the flank at least 0");
    if ((int64_t)m + 2 * (int64_t)flank > PFMSCAN_MAX_WIDTH)
        return fail(ctx, PFMSCAN_E_BADSHAPE, "site sums: width + 2 x flank exceeds PFMSCAN_MAX_WIDTH");
    return PFMSCAN_OK;
}

int pfmscan::site_verdict(pfmscan_ctx *ctx, const int64_t *v, int64_t cell_base, int64_t *first_bad)
{
    if (v[1] != SITE_NONE)
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: the group table does not cover the hits in order, a hit's window leaves "
                                           "the record of its group, or a record lies outside the stream");
    if (v[0] != SITE_NONE) {
        const int64_t at = cell_base + v[0];
        if (first_bad) *first_bad = at;
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: row " + std::to_string(at / 7) + ", column " + std::to_string(at % 7) +
                                               " under a hit is NaN, infinite or negative");
    }
    return PFMSCAN_OK;
}

extern "C" {

int pfmscan_site_sums_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                          const int64_t *d_hit_pos, int64_t n_hits, const int64_t *d_grp_first, const int64_t *d_grp_rec,
                          int64_t n_grp, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, int32_t m,
                          int32_t flank, double *d_sums, uint32_t *d_counts, int64_t *first_bad, void *stream)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    return site_dev(ctx, d_codes, d_profile, profile_dtype, n_pos, d_hit_pos, n_hits, d_grp_first, d_grp_rec, n_grp, d_rec_off,
                    d_rec_len, n_rec, m, flank, d_sums, d_counts, first_bad, stream ? (hipStream_t)stream : ctx->stream);
}

int pfmscan_site_sums_staged(pfmscan_ctx *ctx, int use_codes, int use_profile, const int64_t *hit_pos, int64_t n_hits,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t m, int32_t flank,
                             int64_t capacity, int64_t *grp_rec, double *sums, uint32_t *counts, int64_t *n_grp,
                             int64_t *first_bad)
{
    if (first_bad) *first_bad = -1;
    if (n_grp) *n_grp = 0;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    if (!n_grp) return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL argument");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: no stream is staged");
    if ((use_codes && !ctx->staged_codes) || (use_profile && !ctx->staged_profile))
        return fail(ctx, PFMSCAN_E_BADARG, "site sums: the staged stream lacks the codes or the profile asked for");
    if (!use_codes && !use_profile) return fail(ctx, PFMSCAN_E_BADARG, "site sums: neither codes nor a profile");
    int rc = site_shape(ctx, use_profile != 0, ctx->staged_dtype, m, flank);
    if (rc) return rc;
    if (n_hits < 0 || n_rec < 0 || capacity < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: negative size");
    if ((n_hits > 0 && !hit_pos) || (n_rec > 0 && (!rec_off || !rec_len))) return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL argument");
    std::vector<int64_t> gf, gr;
    if ((rc = site_cut(ctx, hit_pos, n_hits, rec_off, rec_len, n_rec, m, capacity, gf, gr, n_grp))) return rc;
    const int64_t ng = *n_grp;
    if (ng == 0) return PFMSCAN_OK;
    if (!grp_rec || (use_profile && !sums) || (use_codes && !counts)) return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int W = m + 2 * flank;
    const int64_t *d_hit, *d_first, *d_grec, *d_off, *d_len;
    if ((rc = site_upload_tables(ctx, hit_pos, n_hits, gf, gr, rec_off, rec_len, n_rec, &d_hit, &d_first, &d_grec, &d_off, &d_len))) return rc;
    const size_t sum_bytes = (size_t)ng * W * 7 * sizeof(double), cnt_bytes = (size_t)ng * W * 8 * sizeof(uint32_t);
    if (use_profile && (rc = ensure(ctx, ctx->site_sums, sum_bytes))) return rc;
    if (use_codes && (rc = ensure(ctx, ctx->site_counts, cnt_bytes))) return rc;
    rc = site_dev(ctx, use_codes ? static_cast<const uint8_t *>(ctx->codes.p) : nullptr, use_profile ? ctx->profile.p : nullptr,
                  ctx->staged_dtype, ctx->staged_n, d_hit, n_hits, d_first, d_grec, ng, d_off, d_len, n_rec, m, flank,
                  use_profile ? static_cast<double *>(ctx->site_sums.p) : nullptr,
                  use_codes ? static_cast<uint32_t *>(ctx->site_counts.p) : nullptr, first_bad, ctx->stream);
    if (rc) return rc;
    if (use_profile) HIP_TRY(ctx, hipMemcpyAsync(sums, ctx->site_sums.p, sum_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (use_codes) HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->site_counts.p, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::copy(gr.begin(), gr.end(), grp_rec);
    return PFMSCAN_OK;
}

int pfmscan_site_sums_host(pfmscan_ctx *ctx, const uint8_t *codes, const void *profile, int profile_dtype, int64_t n_pos,
                           const int64_t *hit_pos, int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                           int32_t m, int32_t flank, int64_t capacity, int64_t *grp_rec, double *sums, uint32_t *counts,
                           int64_t *n_grp, int64_t *first_bad)
{
    if (first_bad) *first_bad = -1;
    if (n_grp) *n_grp = 0;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    if (!n_grp) return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL argument");
    if (!codes && !profile) return fail(ctx, PFMSCAN_E_BADARG, "site sums: neither codes nor a profile");
    int rc = site_shape(ctx, profile != nullptr, profile_dtype, m, flank);
    if (rc) return rc;
    if (n_pos < 0 || n_hits < 0 || n_rec < 0 || capacity < 0) return fail(ctx, PFMSCAN_E_BADARG, "site sums: negative size");
    if ((n_hits > 0 && !hit_pos) || (n_rec > 0 && (!rec_off || !rec_len))) return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL argument");
    std::vector<int64_t> gf, gr;
    if ((rc = site_cut(ctx, hit_pos, n_hits, rec_off, rec_len, n_rec, m, capacity, gf, gr, n_grp))) return rc;
    for (int64_t r = 0; r < n_rec; ++r)                      // the cuts below rely on it (the device checks it again)
        if (rec_off[r] > n_pos || rec_len[r] > n_pos - rec_off[r])
            return fail(ctx, PFMSCAN_E_BADARG, "site sums: record " + std::to_string(r) + " lies outside the stream");
    const int64_t ng = *n_grp;
    if (ng == 0) return PFMSCAN_OK;
    if (!grp_rec || (profile && !sums) || (codes && !counts)) return fail(ctx, PFMSCAN_E_BADARG, "site sums: NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int W = m + 2 * flank;
    const size_t row_bytes = (size_t)7 * (profile_dtype == PFMSCAN_PROFILE_F32 ? 4 : 8);
    // pieces of whole records, at most `chunk` rows each (a longer record is a piece of its own); a piece without a hit
    // is not uploaded.  Per piece: records [r0, r1), groups [g0, g1)
    int64_t chunk = (int64_t)1 << 24;
    if (const char *e = std::getenv("PFMSCAN_SITES_CHUNK")) chunk = std::max<int64_t>(1, std::atoll(e));
    struct Piece { int64_t r0, r1, g0, g1; };
    std::vector<Piece> pieces;
    int64_t max_rows = 0, max_grp = 0, max_hits = 0;
    for (int64_t r = 0, g = 0; r < n_rec;) {
        const int64_t first = rec_off[r];
        int64_t e = r + 1;
        while (e < n_rec && rec_off[e] + rec_len[e] - first <= chunk) ++e;
        const int64_t g0 = g;
        while (g < ng && gr[(size_t)g] < e) ++g;
        if (g > g0) {
            pieces.push_back({r, e, g0, g});
            max_rows = std::max(max_rows, rec_off[e - 1] + rec_len[e - 1] - first);
            max_grp = std::max(max_grp, g - g0);
            max_hits = std::max(max_hits, gf[(size_t)g] - gf[(size_t)g0]);
        }
        r = e;
    }
    const int64_t n_pieces = (int64_t)pieces.size();
    const int64_t *d_hit, *d_first, *d_grec, *d_off, *d_len;
    if ((rc = site_upload_tables(ctx, hit_pos, n_hits, gf, gr, rec_off, rec_len, n_rec, &d_hit, &d_first, &d_grec, &d_off, &d_len))) return rc;
    const size_t sum_bytes = (size_t)ng * W * 7 * sizeof(double), cnt_bytes = (size_t)ng * W * 8 * sizeof(uint32_t);
    if (profile && (rc = ensure(ctx, ctx->site_sums, sum_bytes))) return rc;
    if (codes && (rc = ensure(ctx, ctx->site_counts, cnt_bytes))) return rc;
    const size_t words = site_blk_words(max_hits, max_grp);
    if ((rc = ensure(ctx, ctx->site_blk, (words + 2 * (size_t)n_pieces) * sizeof(int64_t)))) return rc;
    if (!ctx->copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if (profile && (rc = ensure(ctx, ctx->pipe_profile[i], std::max<size_t>((size_t)max_rows * row_bytes, 16)))) return rc;
        if (codes && (rc = ensure(ctx, ctx->pipe_codes[i], std::max<size_t>((size_t)max_rows, 16)))) return rc;
        if (!ctx->pipe_copied[i]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe_copied[i], hipEventDisableTiming));
        if (!ctx->pipe_scanned[i]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe_scanned[i], hipEventDisableTiming));
    }
    double *d_sums = profile ? static_cast<double *>(ctx->site_sums.p) : nullptr;
    uint32_t *d_counts = codes ? static_cast<uint32_t *>(ctx->site_counts.p) : nullptr;
    int64_t *blk = static_cast<int64_t *>(ctx->site_blk.p);
    int64_t *verdicts = blk + words;
    // the tables are uploaded on the ctx's stream, which also runs every launch; the copy stream only moves the stream's rows
    auto rows_of = [&](int64_t k, int64_t *first) {
        const Piece &p = pieces[(size_t)k];
        *first = rec_off[p.r0];
        return rec_off[p.r1 - 1] + rec_len[p.r1 - 1] - rec_off[p.r0];
    };
    auto send = [&](int64_t k) -> int {
        const int b = (int)(k & 1);
        int64_t first = 0;
        const int64_t rows = rows_of(k, &first);
        if (k >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->pipe_scanned[b], 0));
        if (rows > 0 && profile)
            if (int urc = upload(ctx, ctx->pipe_profile[b].p, static_cast<const unsigned char *>(profile) + (size_t)first * row_bytes,
                                 (size_t)rows * row_bytes, ctx->copy_stream))
                return urc;
        if (rows > 0 && codes)
            if (int urc = upload(ctx, ctx->pipe_codes[b].p, codes + first, (size_t)rows, ctx->copy_stream)) return urc;
        HIP_TRY(ctx, hipEventRecord(ctx->pipe_copied[b], ctx->copy_stream));
        return PFMSCAN_OK;
    };
    if ((rc = send(0))) return rc;
    for (int64_t k = 0; k < n_pieces; ++k) {
        const int b = (int)(k & 1);
        const Piece &p = pieces[(size_t)k];
        int64_t first = 0;
        const int64_t rows = rows_of(k, &first);
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->pipe_copied[b], 0));
        SiteArgs a;
        a.n_pos = rows;
        a.hit_pos = d_hit;
        a.n_hits = n_hits;
        a.grp_first = d_first + p.g0;
        a.grp_rec = d_grec + p.g0;
        a.n_grp = p.g1 - p.g0;
        a.rec_off = d_off;
        a.rec_len = d_len;
        a.n_rec = n_rec;
        a.row_base = first;
        a.hit_lo = gf[(size_t)p.g0];
        a.hit_hi = gf[(size_t)p.g1];
        a.m = m;
        a.flank = flank;
        if ((rc = site_launch(ctx, a, codes ? static_cast<const uint8_t *>(ctx->pipe_codes[b].p) : nullptr,
                              profile ? ctx->pipe_profile[b].p : nullptr, profile_dtype, d_sums ? d_sums + p.g0 * W * 7 : nullptr,
                              d_counts ? d_counts + p.g0 * W * 8 : nullptr, blk, verdicts + 2 * k, ctx->stream)))
            return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->pipe_scanned[b], ctx->stream));
        if (k + 1 < n_pieces && (rc = send(k + 1))) return rc;
    }
    std::vector<int64_t> v((size_t)n_pieces * 2, SITE_NONE);
    HIP_TRY(ctx, hipMemcpyAsync(v.data(), verdicts, v.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t k = 0; k < n_pieces; ++k)                   // pieces are in input order: the first rejected one holds the earliest cell
        if ((rc = site_verdict(ctx, &v[(size_t)k * 2], rec_off[pieces[(size_t)k].r0] * 7, first_bad))) return rc;
    if (profile) HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, sum_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (codes) HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::copy(gr.begin(), gr.end(), grp_rec);
    return PFMSCAN_OK;
}

}  // extern "C"
