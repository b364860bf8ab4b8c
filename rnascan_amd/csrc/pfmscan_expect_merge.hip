// pfmscan_expect_merge.hip -- the records of the expected counts added up exactly on the device (DESIGN.md 5k,
// include/pfmscan.h "expected counts: the records added up on the device").
//
// The expected-count passes leave one matrix [m][8] per record and motif.  Their sum over the records is held in the long
// accumulator of the library site profiles (pfmscan_superacc.hpp): a finite double v > 0 is the integer v / 2^-1074, cut
// into three 32-bit pieces that are added to three consecutive 64-bit limbs.  Integer additions commute and associate, so
// the limbs are the same for every schedule and the adds may be atomics; rounded once (pfmscan_site_acc_round) the sum is
// math.fsum of the cells.  No float atomics, no tolerance: tests/expect_merge_rules.py restates it in Python ints.
//
//   k_exp_merge   a workgroup owns one motif, a tile of MERGE_TILE consecutive cells of its matrix and a range of records.
//                 The tile's 66 limbs x 64 cells lie in LDS (33 KB).  A wave takes every fourth record of the range, a lane
//                 per cell: the 64 lanes read 512 contiguous bytes of the record's matrix and add their pieces to their own
//                 cells with 64-bit LDS atomics, so the lanes of a wave never meet; waves do, on the LDS atomic unit.
//                 MERGE_UNROLL records are loaded before the first is decomposed.  Then every non-zero limb of the tile
//                 goes to d_acc with one 64-bit global atomic: values of one magnitude touch 3 to 5 of the 66 limbs, so a
//                 workgroup sends a few hundred atomics where the naive shape (three global atomics per value, every record
//                 on the same m x 8 addresses) sends three per cell and record.
//                 A NaN, +-inf or negative cell is never decomposed: the smallest record index is kept per lane, reduced in
//                 LDS and sent to d_bad with an unsigned 64-bit atomicMin (-1 is the largest unsigned value: "none").
// Headroom: a value adds at most one piece below 2^32 to a limb, so a limb in LDS stays below records x 2^32 and a raw limb
// of d_acc below 2^63 while an accumulator has taken fewer than 2^31 records: the caller's rule, as for the site profiles.
#include <algorithm>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_occ.hpp"
#include "pfmscan_superacc.hpp"

namespace pfmscan {

constexpr int MERGE_LIMBS = PFMSCAN_SITE_LIMBS;
constexpr int MERGE_BLOCK = 256;
constexpr int MERGE_TILE = 64;                                 // cells of a tile: a lane each
constexpr int MERGE_WAVES = MERGE_BLOCK / MERGE_TILE;          // records a workgroup has in flight per step
constexpr int MERGE_UNROLL = 4;                                // records a wave loads before it decomposes the first
constexpr int64_t MERGE_MIN_RECORDS = 64;                      // records per workgroup at least: the flush walks 4224 limbs
constexpr unsigned long long MERGE_NONE = ~0ull;
static_assert(MERGE_TILE == 64, "a wave of 64 lanes covers a tile");

struct MergeArgs {
    const double *exp;           // [n_rec][n_motifs][ncell]
    int64_t n_rec;
    int64_t per_wg;              // records per workgroup
    int n_motifs, k0;            // motif of blockIdx.y == 0
    int ncell, tiles;            // m * 8, ceil(ncell / MERGE_TILE)
};

__global__ __launch_bounds__(MERGE_BLOCK) void k_exp_merge(const MergeArgs a, unsigned long long *__restrict__ acc,
                                                           unsigned long long *__restrict__ bad)
{
    __shared__ unsigned long long limb[MERGE_LIMBS * MERGE_TILE];
    __shared__ unsigned long long sbad[2];
    const int t = threadIdx.x, lane = t & (MERGE_TILE - 1), wave = t / MERGE_TILE;
    const int64_t chunk = (int64_t)(blockIdx.x / (unsigned)a.tiles);
    const int c0 = (int)(blockIdx.x % (unsigned)a.tiles) * MERGE_TILE, nc = min(MERGE_TILE, a.ncell - c0);
    const int k = a.k0 + (int)blockIdx.y;
    const int64_t r0 = chunk * a.per_wg, r1 = min(r0 + a.per_wg, a.n_rec);
    for (int i = t; i < MERGE_LIMBS * MERGE_TILE; i += MERGE_BLOCK) limb[i] = 0ull;
    if (t < 2) sbad[t] = MERGE_NONE;
    __syncthreads();

    unsigned long long b_inf = MERGE_NONE, b_neg = MERGE_NONE;
    if (lane < nc) {
        const size_t stride = (size_t)a.n_motifs * a.ncell;
        const double *src = a.exp + (size_t)k * a.ncell + c0 + lane;
        for (int64_t r = r0 + wave; r < r1; r += MERGE_WAVES * MERGE_UNROLL) {
            double v[MERGE_UNROLL];
#pragma unroll
            for (int u = 0; u < MERGE_UNROLL; ++u) {
                const int64_t rr = r + u * MERGE_WAVES;
                v[u] = rr < r1 ? src[(size_t)rr * stride] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < MERGE_UNROLL; ++u) {
                const unsigned long long rr = (unsigned long long)(r + u * MERGE_WAVES);
                const unsigned long long bits = (unsigned long long)__double_as_longlong(v[u]);
                const bool nonfinite = ((bits >> 52) & 0x7ffu) == 0x7ffu, negative = v[u] < 0.0;
                if (nonfinite) b_inf = min(b_inf, rr);
                if (negative) b_neg = min(b_neg, rr);
                if (nonfinite || negative || (bits << 1) == 0ull) continue;      // +0.0 and -0.0 have no pieces
                uint32_t piece[3];
                const int first = site_acc_pieces(v[u], piece);
                unsigned long long *dst = limb + first * MERGE_TILE + lane;
                if (piece[0]) atomicAdd(dst, (unsigned long long)piece[0]);
                if (piece[1]) atomicAdd(dst + MERGE_TILE, (unsigned long long)piece[1]);
                if (piece[2]) atomicAdd(dst + 2 * MERGE_TILE, (unsigned long long)piece[2]);
            }
        }
    }
    if (b_inf != MERGE_NONE) atomicMin(&sbad[0], b_inf);
    if (b_neg != MERGE_NONE) atomicMin(&sbad[1], b_neg);
    __syncthreads();
    // a lane that is no cell of the tile has added nothing: a non-zero limb lies inside the motif's ncell cells
    unsigned long long *out = acc + (size_t)k * MERGE_LIMBS * a.ncell + c0;
    for (int i = t; i < MERGE_LIMBS * MERGE_TILE; i += MERGE_BLOCK) {
        const unsigned long long x = limb[i];
        if (x) atomicAdd(out + (size_t)(i / MERGE_TILE) * a.ncell + (i & (MERGE_TILE - 1)), x);
    }
    if (t < 2 && sbad[t] != MERGE_NONE) atomicMin(bad + (size_t)k * 2 + t, sbad[t]);
}

// Records per workgroup.  Enough workgroups to give every CU several (eight), but never fewer than MERGE_MIN_RECORDS records
// each: below that zeroing and walking the tile's 4224 limbs costs more than the records.  The sums do not depend on it.
static int64_t merge_per_wg(const pfmscan_ctx *ctx, int64_t n_rec, int64_t columns)
{
    const int64_t want = std::max<int64_t>(8 * (int64_t)std::max(ctx->n_cu, 1) / std::max<int64_t>(columns, 1), 1);
    const int64_t chunks = std::min(want, (n_rec + MERGE_MIN_RECORDS - 1) / MERGE_MIN_RECORDS);
    return (n_rec + chunks - 1) / chunks;
}

// launches on st, does not wait; rows: the matrix rows of a motif (m, or 4 m for the letter-pair table of two code streams)
static int merge_launch(pfmscan_ctx *ctx, const double *d_exp, int64_t n_rec, int n_motifs, int rows, int zero_first, uint64_t *d_acc,
                        int64_t *d_bad, hipStream_t st)
{
    const int ncell = rows * 8;
    if (zero_first) {
        HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, (size_t)n_motifs * MERGE_LIMBS * ncell * sizeof(uint64_t), st));
        HIP_TRY(ctx, hipMemsetAsync(d_bad, 0xFF, (size_t)n_motifs * 2 * sizeof(int64_t), st));      // -1 everywhere
    }
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    MergeArgs a{};
    a.exp = d_exp;
    a.n_rec = n_rec;
    a.n_motifs = n_motifs;
    a.ncell = ncell;
    a.tiles = (ncell + MERGE_TILE - 1) / MERGE_TILE;
    a.per_wg = merge_per_wg(ctx, n_rec, (int64_t)a.tiles * n_motifs);
    const int64_t chunks = (n_rec + a.per_wg - 1) / a.per_wg;      // below 2^25: n_rec < 2^31, at least 64 records each
    for (int k0 = 0; k0 < n_motifs; k0 += 65535) {
        a.k0 = k0;
        hipLaunchKernelGGL(k_exp_merge, dim3((unsigned)(chunks * a.tiles), (unsigned)std::min(65535, n_motifs - k0)), dim3(MERGE_BLOCK), 0, st, a,
                           (unsigned long long *)d_acc, (unsigned long long *)d_bad);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(ctx, e, "k_exp_merge");
    }
    return PFMSCAN_OK;
}

static int merge_check(pfmscan_ctx *ctx, const char *who, int64_t n_rec, int n_motifs, int m)
{
    if (n_rec < 0 || n_motifs < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": negative size");
    if (n_rec > 0x7FFFFFFF) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": an accumulator takes fewer than 2^31 records");
    if (m < 1 || m > PFMSCAN_MAX_M)
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": width " + std::to_string(m) + " outside 1 .. PFMSCAN_MAX_M (" + std::to_string(PFMSCAN_MAX_M) + ")");
    return PFMSCAN_OK;
}

int exp_merge_home(pfmscan_ctx *ctx, const char *who, const ExpMergeOut *out, int n_out, int64_t n_rec, int n_motifs, int m, const double *d_occ,
                   double *occ, const int64_t *d_windows, int64_t *windows)
{
    int rc;
    if ((rc = merge_check(ctx, who, n_rec, n_motifs, m))) return rc;
    const size_t verdicts = (size_t)n_motifs * 2;
    std::vector<size_t> at(n_out + 1, 0);                          // where output i's words, then its verdicts, lie in ctx->exp_acc
    for (int i = 0; i < n_out; ++i) {
        if (out[i].rows != m && out[i].rows != 4 * m)             // a matrix, or the letter-pair table of two code streams
            return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": an output of " + std::to_string(out[i].rows) + " rows: the width or 4 times the width");
        at[i + 1] = at[i] + (out[i].d_exp ? (size_t)n_motifs * MERGE_LIMBS * out[i].rows * 8 + verdicts : 0);
    }
    if ((rc = ensure(ctx, ctx->exp_acc, std::max<size_t>(at[n_out] * 8, 16)))) return rc;
    std::vector<uint64_t> home(at[n_out]);
    for (int i = 0; i < n_out; ++i) {
        if (!out[i].d_exp) continue;
        const size_t one = at[i + 1] - at[i];
        uint64_t *d_acc = (uint64_t *)ctx->exp_acc.p + at[i];
        if ((rc = merge_launch(ctx, out[i].d_exp, n_rec, n_motifs, out[i].rows, 1, d_acc, (int64_t *)(d_acc + one - verdicts), ctx->stream))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(home.data() + at[i], d_acc, one * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (occ) HIP_TRY(ctx, hipMemcpyAsync(occ, d_occ, (size_t)n_rec * n_motifs * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (windows) HIP_TRY(ctx, hipMemcpyAsync(windows, d_windows, (size_t)n_rec * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_out; ++i) {
        if (!out[i].d_exp) continue;
        const uint64_t *raw = home.data() + at[i];
        const size_t words = at[i + 1] - at[i] - verdicts;
        if (pfmscan_site_acc_add(out[i].acc, raw, n_motifs, (int64_t)out[i].rows * 8) != PFMSCAN_OK)
            return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": the top limb of an accumulator overflows");
        for (size_t j = 0; j < verdicts; ++j) out[i].bad[j] = (int64_t)raw[words + j];
    }
    return PFMSCAN_OK;
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_expect_merge_dev(pfmscan_ctx *ctx, const double *d_exp, int64_t n_rec, int n_motifs, int m, int zero_first, uint64_t *d_acc,
                             int64_t *d_bad)
{
    const char *who = "pfmscan_expect_merge_dev";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = merge_check(ctx, who, n_rec, n_motifs, m)) return rc;
    if (n_motifs > 0 && (!d_acc || !d_bad)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL accumulators or verdicts");
    if (n_motifs > 0 && n_rec > 0 && !d_exp) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL matrices");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return merge_launch(ctx, d_exp, n_rec, n_motifs, m, zero_first, d_acc, d_bad, ctx->stream);
}

}  // extern "C"
