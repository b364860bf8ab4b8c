// pfmscan_sites_letters.hip -- site profiles on LETTER streams: the letters of one or two code streams counted under the
// hits of every motif of one width, per column and per PAIR of letters (include/pfmscan.h, "site profiles on letter
// streams").  The reference's PFM builder counts letters under aligned windows (struct_pfm_from_aligned,
// average_structure.py:28-42) and normalises per position (norm_pfm, pfmutil.py:136-151); the joint table
// joint[k][j][a][b] holds those counts for both streams at once, and its marginals are the two count tables.
//
// All of it is integer counting: additions commute and associate, so the table is a function of the input alone whatever
// the schedule (the argument of pfmscan_sites_lib.hip).  LDS atomics and 64-bit global integer atomics, no float atomics.
//
//   k_site_joint   one LANE owns a hit, a workgroup owns a contiguous SLICE of the motif-major hit list.  The slice is walked
//                  in runs of one motif (the list does not descend: a run ends where a binary search finds the next motif)
//                  and the W columns in tiles of PFMSCAN_SITE_JOINT_COLS.  Per run and tile: the workgroup zeroes an LDS
//                  table uint32 [COLS][64], every lane finds its hit's record by binary search of rec_off, walks the
//                  tile's columns that lie inside the record and adds 1 to cell (codes[x] & 7) * 8 + (codes2[x] & 7)
//                  with an LDS atomic; then the non-zero cells go to the motif's table with one 64-bit atomicAdd each.
//                  A slice holds at most JOINT_SLICE_MAX = 2^24 hits and a hit adds at most 1 to a cell of a tile, so
//                  an LDS cell stays below 2^24 and cannot wrap.
//                  The validity of every hit of the slice is judged first (a position outside the stream, a window that
//                  leaves its record, a motif index outside [0, n_motifs), a motif smaller than the one before): the
//                  smallest bad hit index per workgroup goes to blk[], k_site_verdict (pfmscan_sites.hpp) reduces it.
//                  Whatever the tables hold, a load happens only inside the buffers -- a code only for a row inside a
//                  record that lies inside the stream -- and an add only inside the table of a motif in [0, n_motifs).
//
// No register array is indexed at run time (the histogram lives in LDS), no kernel uses scratch, no workgroup waits on
// another, 64-bit positions and element indices throughout.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "pfmscan_sites.hpp"

using namespace pfmscan;

namespace {

constexpr int JOINT_BLOCK = 256;
constexpr int JOINT_COLS = PFMSCAN_SITE_JOINT_COLS;
constexpr int64_t JOINT_SLICE_MAX = (int64_t)1 << 24;        // hits of one slice: an LDS cell stays below 2^24
constexpr int64_t JOINT_SLICE_MIN = JOINT_BLOCK;             // default slices are at least one hit per lane (profiles/sites_letters/NOTES.md)

struct SiteJointArgs {
    const uint8_t *codes, *codes2;                           // either may be NULL: its index is 0
    int64_t n_pos;
    const int64_t *hit_pos;                                  // [n_hits] motif-major
    const int32_t *hit_motif;                                // [n_hits] or NULL: one motif
    int64_t n_hits;
    const int64_t *rec_off, *rec_len;                        // [n_rec]
    int64_t n_rec;
    int64_t slice;                                           // hits per workgroup
    int n_motifs, m, flank;
};

// the record a position lies in: the last one that starts at or before p; [roff, rend) inside the stream, or false
__device__ inline bool joint_record(const SiteJointArgs &a, int64_t p, int64_t &roff, int64_t &rend)
{
    if (p < 0 || p >= a.n_pos) return false;
    int64_t lo = 0, hi = a.n_rec;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.rec_off[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return false;
    const int64_t off = a.rec_off[lo - 1], len = a.rec_len[lo - 1];
    if (!site_inside(off, len, a.n_pos) || p >= off + len) return false;
    roff = off;
    rend = off + len;
    return true;
}

__global__ __launch_bounds__(JOINT_BLOCK) void k_site_joint(SiteJointArgs a, unsigned long long *__restrict__ out,
                                                            int64_t *__restrict__ blk)
{
    __shared__ unsigned int tab[JOINT_COLS * 64];
    __shared__ int64_t sh[JOINT_BLOCK];
    const int t = threadIdx.x;
    const int F = a.flank, W = a.m + 2 * F;
    const int64_t s0 = (int64_t)blockIdx.x * a.slice, s1 = min(s0 + a.slice, a.n_hits);

    // the verdict on this slice's hits
    int64_t key = SITE_NONE;
    for (int64_t i = s0 + t; i < s1; i += JOINT_BLOCK) {
        const int64_t p = a.hit_pos[i];
        const int64_t k = a.hit_motif ? (int64_t)a.hit_motif[i] : 0;
        int64_t roff = 0, rend = 0;
        bool bad = k < 0 || k >= a.n_motifs || (a.hit_motif && i > 0 && (int64_t)a.hit_motif[i - 1] > k);
        if (!bad) bad = !joint_record(a, p, roff, rend) || (int64_t)a.m > rend - p;
        if (bad) key = min(key, i);
    }
    key = site_block_min(key, sh);
    if (t == 0) blk[blockIdx.x] = key;

    // runs of one motif [s, e) inside the slice
    for (int64_t s = s0; s < s1;) {
        const int64_t k = a.hit_motif ? (int64_t)a.hit_motif[s] : 0;
        int64_t e = s1;
        if (a.hit_motif) {                                   // the first hit behind s whose motif is larger (the list does not descend)
            int64_t lo = s + 1, hi = s1;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if ((int64_t)a.hit_motif[mid] <= k) lo = mid + 1;
                else hi = mid;
            }
            e = lo;
        }
        if (k >= 0 && k < a.n_motifs) {
            for (int t0 = 0; t0 < W; t0 += JOINT_COLS) {
                const int nc = min(JOINT_COLS, W - t0);
                for (int c = t; c < nc * 64; c += JOINT_BLOCK) tab[c] = 0u;
                __syncthreads();
                for (int64_t i = s + t; i < e; i += JOINT_BLOCK) {
                    if (a.hit_motif && (int64_t)a.hit_motif[i] != k) continue;      // a broken list: judged above, counted nowhere
                    const int64_t p = a.hit_pos[i];
                    int64_t roff = 0, rend = 0;
                    if (!joint_record(a, p, roff, rend)) continue;
                    // columns j in [t0, t0 + nc) whose row x = p - F + j lies inside the record
                    const int64_t x0 = p - F;
                    const int64_t jlo = max((int64_t)t0, roff - x0), jhi = min((int64_t)(t0 + nc), rend - x0);
                    for (int64_t j = jlo; j < jhi; ++j) {
                        const int64_t x = x0 + j;
                        const unsigned int ca = a.codes ? (unsigned int)(a.codes[x] & 7u) : 0u;
                        const unsigned int cb = a.codes2 ? (unsigned int)(a.codes2[x] & 7u) : 0u;
                        atomicAdd(&tab[(int)(j - t0) * 64 + (int)(ca * 8u + cb)], 1u);
                    }
                }
                __syncthreads();
                unsigned long long *dst = out + ((size_t)k * W + t0) * 64;
                for (int c = t; c < nc * 64; c += JOINT_BLOCK) {
                    const unsigned int v = tab[c];
                    if (v) atomicAdd(dst + c, (unsigned long long)v);
                }
                __syncthreads();
            }
        }
        s = e;
    }
}

int64_t joint_slice(const pfmscan_ctx *ctx, int64_t n_hits)
{
    // PFMSCAN_SITE_JOINT_SLICE in the environment overrides (the tests cut short lists into several slices with it); the
    // table does not depend on it
    if (const char *env = std::getenv("PFMSCAN_SITE_JOINT_SLICE")) {
        char *end = nullptr;
        const long long v = std::strtoll(env, &end, 10);
        if (end != env && v >= 1) return std::min<int64_t>(v, JOINT_SLICE_MAX);
    }
    // about four workgroups per CU, whole multiples of the workgroup
    const int64_t groups = 4 * (int64_t)std::max(ctx->n_cu, 1);
    int64_t slice = (n_hits + groups - 1) / groups;
    slice = (slice + JOINT_BLOCK - 1) / JOINT_BLOCK * JOINT_BLOCK;
    return std::min(std::max(slice, JOINT_SLICE_MIN), JOINT_SLICE_MAX);
}

int joint_shape(pfmscan_ctx *ctx, int64_t n_hits, int64_t n_rec, int32_t n_motifs, int32_t m, int32_t flank)
{
    const int rc = site_shape(ctx, false, PFMSCAN_PROFILE_NONE, m, flank);
    if (rc) return rc;
    if (n_hits < 0 || n_rec < 0 || n_motifs < 0) return fail(ctx, PFMSCAN_E_BADARG, "site joint: negative size");
    return PFMSCAN_OK;
}

int joint_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_hit_pos,
              const int32_t *d_hit_motif, int64_t n_hits, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec,
              int32_t n_motifs, int32_t m, int32_t flank, uint64_t *d_joint, hipStream_t st)
{
    int rc = joint_shape(ctx, n_hits, n_rec, n_motifs, m, flank);
    if (rc) return rc;
    if (n_pos < 0) return fail(ctx, PFMSCAN_E_BADARG, "site joint: negative size");
    if (!d_codes && !d_codes2) return fail(ctx, PFMSCAN_E_BADARG, "site joint: neither code stream");
    if (n_motifs > 0 && !d_joint) return fail(ctx, PFMSCAN_E_BADARG, "site joint: no output buffer");
    if (n_hits > 0 && (!d_hit_pos || (n_rec > 0 && (!d_rec_off || !d_rec_len)))) return fail(ctx, PFMSCAN_E_BADARG, "site joint: NULL buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int W = m + 2 * flank;
    if (n_motifs > 0) HIP_TRY(ctx, hipMemsetAsync(d_joint, 0, (size_t)n_motifs * W * 64 * sizeof(uint64_t), st));
    if (n_hits == 0) return PFMSCAN_OK;
    const int64_t slice = joint_slice(ctx, n_hits);
    const int64_t nb = (n_hits + slice - 1) / slice;
    if (nb > INT_MAX) return fail(ctx, PFMSCAN_E_BADSHAPE, "site joint: too many slices for one launch");
    if ((rc = ensure(ctx, ctx->site_blk, ((size_t)nb + 2) * sizeof(int64_t)))) return rc;
    int64_t *blk = static_cast<int64_t *>(ctx->site_blk.p), *d_verdict = blk + nb;
    SiteJointArgs a;
    a.codes = d_codes;
    a.codes2 = d_codes2;
    a.n_pos = n_pos;
    a.hit_pos = d_hit_pos;
    a.hit_motif = d_hit_motif;
    a.n_hits = n_hits;
    a.rec_off = d_rec_off;
    a.rec_len = d_rec_len;
    a.n_rec = n_rec;
    a.slice = slice;
    a.n_motifs = n_motifs;
    a.m = m;
    a.flank = flank;
    hipLaunchKernelGGL(k_site_joint, dim3((unsigned)nb), dim3(JOINT_BLOCK), 0, st, a, reinterpret_cast<unsigned long long *>(d_joint), blk);
    hipLaunchKernelGGL(k_site_verdict, dim3(1), dim3(SITE_VERDICT_BLOCK), 0, st, blk, (int64_t)0, blk, nb, d_verdict);
    HIP_TRY(ctx, hipGetLastError());
    int64_t v[2] = {SITE_NONE, SITE_NONE};
    HIP_TRY(ctx, hipMemcpyAsync(v, d_verdict, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (v[1] != SITE_NONE)
        return fail(ctx, PFMSCAN_E_BADARG, "site joint: hit " + std::to_string(v[1]) + " of the motif-major list lies outside the "
                                           "stream, its window leaves its record, its motif index is no motif or is smaller "
                                           "than the one before");
    return PFMSCAN_OK;
}

}  // namespace

extern "C" {

int pfmscan_site_joint_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos,
                           const int64_t *d_hit_pos, const int32_t *d_hit_motif, int64_t n_hits, const int64_t *d_rec_off,
                           const int64_t *d_rec_len, int64_t n_rec, int32_t n_motifs, int32_t m, int32_t flank, uint64_t *d_joint,
                           void *stream)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    return joint_dev(ctx, d_codes, d_codes2, n_pos, d_hit_pos, d_hit_motif, n_hits, d_rec_off, d_rec_len, n_rec, n_motifs, m, flank,
                     d_joint, stream ? (hipStream_t)stream : ctx->stream);
}

int pfmscan_site_joint_staged(pfmscan_ctx *ctx, int use_codes, int use_codes2, const int64_t *hit_pos, const int32_t *hit_motif,
                              int64_t n_hits, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int32_t n_motifs,
                              int32_t m, int32_t flank, uint64_t *joint)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, "site joint: no stream is staged");
    if (!use_codes && !use_codes2) return fail(ctx, PFMSCAN_E_BADARG, "site joint: neither code stream");
    if ((use_codes && !ctx->staged_codes) || (use_codes2 && !ctx->staged_codes2))
        return fail(ctx, PFMSCAN_E_BADARG, "site joint: the staged stream lacks a code stream asked for (pfmscan_stage, pfmscan_stage_codes2)");
    int rc = joint_shape(ctx, n_hits, n_rec, n_motifs, m, flank);
    if (rc) return rc;
    if ((n_hits > 0 && !hit_pos) || (n_rec > 0 && (!rec_off || !rec_len)) || (n_motifs > 0 && !joint))
        return fail(ctx, PFMSCAN_E_BADARG, "site joint: NULL argument");
    const int W = m + 2 * flank;
    const size_t words = (size_t)n_motifs * W * 64;
    if (n_hits == 0 || n_motifs == 0) {
        if (n_hits > 0) return fail(ctx, PFMSCAN_E_BADARG, "site joint: hits but no motif");
        std::fill(joint, joint + words, uint64_t(0));
        return PFMSCAN_OK;
    }
    // (position, motif) order, as the library scans return their hits -> motif-major
    std::vector<int64_t> pos;
    std::vector<int32_t> motif;
    if (hit_motif) {
        std::vector<int64_t> order((size_t)n_hits);
        if (pfmscan_site_order_lib(hit_pos, hit_motif, n_hits, n_motifs, order.data()))
            return fail(ctx, PFMSCAN_E_BADARG, "site joint: a hit's motif index is no motif of the library");
        pos.resize((size_t)n_hits);
        motif.resize((size_t)n_hits);
        for (int64_t h = 0; h < n_hits; ++h) {
            pos[(size_t)h] = hit_pos[order[(size_t)h]];
            motif[(size_t)h] = hit_motif[order[(size_t)h]];
        }
        hit_pos = pos.data();
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // host tables -> ctx->site_tab: hit_pos | rec_off | rec_len | hit_motif (int32, last: the int64 tables stay aligned)
    if ((rc = ensure(ctx, ctx->site_tab, (size_t)(n_hits + 2 * n_rec) * sizeof(int64_t) + (size_t)n_hits * sizeof(int32_t) + 16))) return rc;
    int64_t *d_pos = static_cast<int64_t *>(ctx->site_tab.p), *d_off = d_pos + n_hits, *d_len = d_off + n_rec;
    int32_t *d_motif = reinterpret_cast<int32_t *>(d_len + n_rec);
    if ((rc = upload(ctx, d_pos, hit_pos, (size_t)n_hits * 8, ctx->stream))) return rc;
    if (n_rec > 0 && (rc = upload(ctx, d_off, rec_off, (size_t)n_rec * 8, ctx->stream))) return rc;
    if (n_rec > 0 && (rc = upload(ctx, d_len, rec_len, (size_t)n_rec * 8, ctx->stream))) return rc;
    if (hit_motif && (rc = upload(ctx, d_motif, motif.data(), (size_t)n_hits * 4, ctx->stream))) return rc;
    if ((rc = ensure(ctx, ctx->site_counts, std::max<size_t>(words * 8, 16)))) return rc;
    rc = joint_dev(ctx, use_codes ? static_cast<const uint8_t *>(ctx->codes.p) : nullptr,
                   use_codes2 ? static_cast<const uint8_t *>(ctx->codes2.p) : nullptr, ctx->staged_n, d_pos,
                   hit_motif ? d_motif : nullptr, n_hits, d_off, d_len, n_rec, n_motifs, m, flank,
                   static_cast<uint64_t *>(ctx->site_counts.p), ctx->stream);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(joint, ctx->site_counts.p, words * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFMSCAN_OK;
}

}  // extern "C"
