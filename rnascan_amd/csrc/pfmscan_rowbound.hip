// pfmscan_rowbound.hip -- the ROW BOUND of a profile stream: the largest fp64 row sum over the rows a scorable window can
// touch, or +inf when one of them breaks the promise "finite and non-negative".  gfx950.
//
// It is the S of pfmscan_exact.hpp's library bound: a structure score is at most S times the sum of the PSSM's row
// maxima, which turns a joint threshold on LogOdds.SeqStruct (rnascan.py:416-434) into a finite letters threshold for
// k_library's credit tables (pfmscan_library_hits_sum_*).
//
//   result = max over positions p with (codes[p] & 7) != 7 of  ((((((r0 + r1) + r2) + r3) + r4) + r5) + r6)
// in fp64 (float32 rows widened first), +inf if such a row holds a NaN, an infinite or a negative entry, 0 when no row
// counts.  Rows under code 7 (record separators, foreign letters) are skipped: every window covering one scores NaN on
// the sequence side (_pwm.c:61-66), so no hit depends on them.  codes == NULL: every row counts.
//
// A maximum does not depend on the order it is taken in: per-workgroup partials and one final workgroup, no float atomics,
// one defined bit pattern (comparisons are `x > best`, so a row of -0.0 entries leaves +0.0).
//
// A pure read stream: a tile is 256 rows = 7168 / 14336 bytes, a multiple of 16, so every tile of a 16-byte aligned
// stream starts on a vector boundary; the lanes load the tile as aligned 16-byte vectors into LDS (rows are 28 / 56
// bytes: not vector aligned themselves) and each lane sums one row from there.
#include <math.h>

#include "pfmscan_ctx.hpp"

namespace pfmscan {

constexpr int RB_BLOCK = 256;                    // lanes of a workgroup = rows of a tile
constexpr int RB_FINAL_BLOCK = 256;

// the aligned 16 bytes at byte_off; the stream's last vector may be cut short by up to 12 bytes
__device__ inline uint4 rb_load(const unsigned char *base, int64_t byte_off, int64_t total_bytes)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (byte_off + 16 <= total_bytes) {
        v = *reinterpret_cast<const uint4 *>(base + byte_off);
    } else {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(base + byte_off);
        const int64_t n = (total_bytes - byte_off) / 4;
        if (n > 0) v.x = p[0];
        if (n > 1) v.y = p[1];
        if (n > 2) v.z = p[2];
    }
    return v;
}

__device__ inline double rb_block_max(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s && sh[t + s] > sh[t]) sh[t] = sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

template <typename T>
__global__ __launch_bounds__(RB_BLOCK) void k_row_bound(const uint8_t *__restrict__ codes, const unsigned char *__restrict__ profile,
                                                        int64_t n_pos, double *__restrict__ part)
{
    constexpr int RBYTES = 7 * (int)sizeof(T);               // bytes of a row
    constexpr int NVEC = RB_BLOCK * RBYTES / 16;             // vectors of a tile: 448 (float), 896 (double)
    constexpr int NV = (NVEC + RB_BLOCK - 1) / RB_BLOCK;     // ... per lane: 2 / 4
    __shared__ uint4 tile[NVEC];
    __shared__ double sh[RB_BLOCK];
    const int t = threadIdx.x;
    const int64_t n_tiles = (n_pos + RB_BLOCK - 1) / RB_BLOCK;
    const int64_t total = n_pos * RBYTES;
    double best = 0.0;
    for (int64_t k = blockIdx.x; k < n_tiles; k += gridDim.x) {
        const int64_t row0 = k * RB_BLOCK;
        const int n = (int)min((int64_t)RB_BLOCK, n_pos - row0);
        const int64_t first = row0 * RBYTES, end = first + (int64_t)n * RBYTES;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = t + j * RB_BLOCK;
            const int64_t b = first + (int64_t)i * 16;
            if (i < NVEC) tile[i] = b < end ? rb_load(profile, b, total) : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        if (t < n && (!codes || (codes[row0 + t] & 7u) != 7u)) {
            const T *row = reinterpret_cast<const T *>(tile) + t * 7;
            double s = 0.0;
            bool bad = false;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const double x = (double)row[c];
                s = c == 0 ? x : s + x;
                bad = bad || !(x >= 0.0 && x < INFINITY);
            }
            if (bad) s = INFINITY;
            if (s > best) best = s;
        }
        __syncthreads();
    }
    const double m = rb_block_max(best, sh);
    if (t == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(RB_FINAL_BLOCK) void k_row_bound_final(const double *__restrict__ part, int n_part, double *__restrict__ out)
{
    __shared__ double sh[RB_FINAL_BLOCK];
    double best = 0.0;
    for (int i = threadIdx.x; i < n_part; i += RB_FINAL_BLOCK)
        if (part[i] > best) best = part[i];
    const double m = rb_block_max(best, sh);
    if (threadIdx.x == 0) *out = m;
}

// partials + final on `st`; d_out may be any device double
static int row_bound_launch(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                            double *d_out, hipStream_t st)
{
    const int64_t n_tiles = (n_pos + RB_BLOCK - 1) / RB_BLOCK;
    const int grid = (int)std::min<int64_t>(n_tiles, (int64_t)std::max(ctx->n_cu, 1) * 8);
    int rc = ensure(ctx, ctx->rb_part, (size_t)std::max(ctx->n_cu, 1) * 8 * sizeof(double) + 16);
    if (rc) return rc;
    double *part = (double *)ctx->rb_part.p;
    if (grid > 0) {
        const unsigned char *prof = reinterpret_cast<const unsigned char *>(d_profile);
        if (profile_dtype == PFMSCAN_PROFILE_F64)
            hipLaunchKernelGGL(k_row_bound<double>, dim3((unsigned)grid), dim3(RB_BLOCK), 0, st, d_codes, prof, n_pos, part);
        else
            hipLaunchKernelGGL(k_row_bound<float>, dim3((unsigned)grid), dim3(RB_BLOCK), 0, st, d_codes, prof, n_pos, part);
        HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_row_bound_final, dim3(1), dim3(RB_FINAL_BLOCK), 0, st, part, grid, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return PFMSCAN_OK;
}

int staged_row_bound(pfmscan_ctx *ctx, double *row_sum_max)
{
    if (ctx->row_bound_serial == ctx->stage_serial) {
        *row_sum_max = ctx->row_bound;
        return PFMSCAN_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure(ctx, ctx->rb_part, (size_t)std::max(ctx->n_cu, 1) * 8 * sizeof(double) + 16);
    if (rc) return rc;
    double *d_out = (double *)ctx->rb_part.p + (size_t)std::max(ctx->n_cu, 1) * 8;       // the slot behind the partials
    if ((rc = row_bound_launch(ctx, ctx->staged_codes ? (const uint8_t *)ctx->codes.p : nullptr, ctx->profile.p, ctx->staged_dtype,
                               ctx->staged_n, d_out, ctx->stream)))
        return rc;
    double v = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(&v, d_out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->row_bound = v;
    ctx->row_bound_serial = ctx->stage_serial;
    *row_sum_max = v;
    return PFMSCAN_OK;
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_profile_row_bound_dev(pfmscan_ctx *ctx, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                  double *d_out, void *stream)
{
    if (!ctx || !d_out) return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_profile_row_bound_dev: NULL argument");
    if (n_pos < 0) return fail(ctx, PFMSCAN_E_BADARG, "negative n_pos");
    if (profile_dtype != PFMSCAN_PROFILE_F32 && profile_dtype != PFMSCAN_PROFILE_F64)
        return fail(ctx, PFMSCAN_E_BADARG, "profile_dtype must be F32 or F64");
    if (n_pos > 0 && !d_profile) return fail(ctx, PFMSCAN_E_BADARG, "profile is NULL");
    if (misaligned(d_profile)) return fail(ctx, PFMSCAN_E_BADSHAPE, "stream base pointers must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return row_bound_launch(ctx, d_codes, d_profile, profile_dtype, n_pos, d_out, stream ? (hipStream_t)stream : ctx->stream);
}

int pfmscan_profile_row_bound_staged(pfmscan_ctx *ctx, double *row_sum_max)
{
    if (!ctx || !row_sum_max) return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_profile_row_bound_staged: NULL argument");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, "no stream staged (call pfmscan_stage first)");
    if (!ctx->staged_profile && ctx->staged_n > 0) return fail(ctx, PFMSCAN_E_BADARG, "no profile is staged");
    if (ctx->staged_n == 0) {
        *row_sum_max = 0.0;
        return PFMSCAN_OK;
    }
    return staged_row_bound(ctx, row_sum_max);
}

}  // extern "C"
