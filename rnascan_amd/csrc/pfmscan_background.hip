// pfmscan_background.hip -- per-record column sums of an averaged-structure profile stream: the counts behind the
// structure background of an averaged-structure input.
//
// compute_background (rnascan.py:440-465) counts the letters of every record; for a profile the count of letter c is the
// sum of column c over every row (the expected number of that letter).  A background feeds every PSSM cell, so the sums
// must come out with the same bits however the stream was cut into batches, chunks or ranks.  Hence:
//
//   * the device produces PER-RECORD sums, double [n_rec][7], each a function of that record's rows alone (the host
//     combines records with math.fsum, which is exactly rounded and so independent of order);
//   * inside a record the order of ADDITIONS is anchored at the record's first row, whatever the order of LOADS:
//       piece p          rows [p * BG_PIECE, min((p + 1) * BG_PIECE, L)) of the record
//       lane t of a piece  acc = 0.0; acc += row[t]; acc += row[t + 256]; ...          (fp32 rows widened first)
//       wave w           lanes 64 w .. 64 w + 63 folded as a[i] += a[i + s] for s = 32, 16, 8, 4, 2, 1
//       piece            ((wave 0 + wave 1) + wave 2) + wave 3
//       record           piece 0, then += piece 1, += piece 2, ...                        (0.0 for an empty record)
//     tests/background_rules.py restates this in numpy; the kernels equal it bit for bit.
//
//   k_bg_pieces    one workgroup per piece.  Rows are 28 / 56 bytes, so they are not 16-byte aligned: a tile of 256 rows
//                  is fetched as the aligned 16-byte vectors that cover it (anchored at the stream, coalesced), parked in
//                  LDS, and every lane reads its own row from LDS at the conflict-free stride of 7 (14) dwords.  The next
//                  tile's vectors are in flight while the current one is added.  The validity check (finite, >= 0) rides
//                  along: the smallest bad flat element index per workgroup.
//   k_bg_records   one lane per record: the record table is consistent, and the record's pieces summed in order.
//   k_bg_verdict   one workgroup: the smallest key of either kind.
//
// A piece's workgroup is found without a prefix sum over the records: piece p of record r sits in slot
// rec_off[r] / BG_PIECE + r + p, which is strictly increasing over (r, p) because a record's rows and its separator lie
// before the next record; slots that hold no piece (at most one per record) return at once.  No global atomics, no
// workgroup waits on another, every load is bounded by the stream and the tables whatever they hold.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"

using namespace pfmscan;

namespace {

constexpr int BG_BLOCK = 256;                    // lanes of a workgroup = rows of a tile
constexpr int BG_WAVES = BG_BLOCK / 64;
constexpr int BG_PIECE = 2048;                   // rows of a piece (8 tiles)
constexpr int BG_REC_BLOCK = 256;
constexpr int BG_VERDICT_BLOCK = 1024;
constexpr int64_t BG_NONE = INT64_MAX;

struct BgArgs {
    const unsigned char *profile;                // [n_pos][7] float or double, 16-byte aligned
    int64_t n_pos;
    const int64_t *rec_off, *rec_len;            // [n_rec]; row of a record in `profile` = rec_off[r] - row_base
    int64_t n_rec, row_base;
    int64_t n_slots;                             // n_pos / BG_PIECE + n_rec
};

__device__ inline int64_t bg_block_min(int64_t v, int64_t *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = min(sh[t], sh[t + s]);
        __syncthreads();
    }
    return sh[0];
}

// record r lies inside the stream
__device__ inline bool bg_inside(int64_t off, int64_t len, int64_t n_pos)
{
    return off >= 0 && len >= 0 && off <= n_pos && len <= n_pos - off;
}

// the aligned 16 bytes at byte_off; the stream's last vector may be cut short by up to 12 bytes
__device__ inline uint4 bg_load(const unsigned char *base, int64_t byte_off, int64_t total_bytes)
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

template <typename T>
__global__ __launch_bounds__(BG_BLOCK) void k_bg_pieces(BgArgs a, double *__restrict__ part, int64_t *__restrict__ blk)
{
    constexpr int RB = 7 * (int)sizeof(T);                   // bytes of a row
    constexpr int NVEC = BG_BLOCK * RB / 16 + 1;             // aligned vectors that cover a tile wherever it starts
    constexpr int NV = (NVEC + BG_BLOCK - 1) / BG_BLOCK;     // ... per lane: 2 (float), 4 (double)
    __shared__ uint4 tile[NVEC];
    __shared__ double wsum[BG_WAVES][7];
    __shared__ int64_t sh[BG_BLOCK];
    const int t = threadIdx.x;
    const int64_t s = blockIdx.x;
    // the record of slot s: the last r with rec_off[r] / BG_PIECE + r <= s (workgroup-uniform)
    int64_t lo = 0, hi = a.n_rec;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const int64_t o = a.rec_off[mid] - a.row_base;
        if ((o < 0 ? -1 : o / BG_PIECE) + mid <= s) lo = mid + 1;
        else hi = mid;
    }
    const int64_t r = lo - 1;
    int64_t off = 0, len = 0, p = 0;
    bool work = r >= 0;
    if (work) {
        off = a.rec_off[r] - a.row_base;
        len = a.rec_len[r];
        work = bg_inside(off, len, a.n_pos);
        p = s - (off / BG_PIECE + r);
        work = work && p >= 0 && p < (len + BG_PIECE - 1) / BG_PIECE;
    }
    if (!work) {                                             // a slot without a piece
        if (t == 0) blk[s] = BG_NONE;
        return;
    }
    const int64_t row0 = off + p * BG_PIECE;
    const int nrows = (int)min((int64_t)BG_PIECE, len - p * BG_PIECE);
    const int ntiles = (nrows + BG_BLOCK - 1) / BG_BLOCK;
    const int64_t total = a.n_pos * RB;

    uint4 v[NV];
    auto fetch = [&](int k) {
        const int64_t first = (row0 + (int64_t)k * BG_BLOCK) * RB;
        const int64_t end = first + (int64_t)min(BG_BLOCK, nrows - k * BG_BLOCK) * RB;
        const int64_t base = first & ~(int64_t)15;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t b = base + (int64_t)(t + j * BG_BLOCK) * 16;
            v[j] = b < end ? bg_load(a.profile, b, total) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    fetch(0);
    double acc[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[c] = 0.0;
    int64_t key = BG_NONE;
    for (int k = 0; k < ntiles; ++k) {
        const int64_t trow = row0 + (int64_t)k * BG_BLOCK;
        const int n = min(BG_BLOCK, nrows - k * BG_BLOCK);
        const int shift = (int)((trow * RB) & 15) / (int)sizeof(T);
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (t + j * BG_BLOCK < NVEC) tile[t + j * BG_BLOCK] = v[j];
        __syncthreads();
        if (k + 1 < ntiles) fetch(k + 1);
        if (t < n) {
            const T *row = reinterpret_cast<const T *>(tile) + t * 7 + shift;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const double x = (double)row[c];
                acc[c] += x;
                if (!(x >= 0.0 && x < INFINITY)) key = min(key, (trow + t) * 7 + c);
            }
        }
        __syncthreads();
    }
    // lanes -> wave -> piece, in the fixed order of the header comment
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        double x = acc[c];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
        if ((t & 63) == 0) wsum[t >> 6][c] = x;
    }
    __syncthreads();
    if (t < 7) part[s * 7 + t] = ((wsum[0][t] + wsum[1][t]) + wsum[2][t]) + wsum[3][t];
    const int64_t m = bg_block_min(key, sh);
    if (t == 0) blk[s] = m;
}

__global__ __launch_bounds__(BG_REC_BLOCK) void k_bg_records(BgArgs a, const double *__restrict__ part,
                                                            double *__restrict__ sums, int64_t *__restrict__ blk)
{
    __shared__ int64_t sh[BG_REC_BLOCK];
    const int64_t r = (int64_t)blockIdx.x * BG_REC_BLOCK + threadIdx.x;
    bool bad = false;
    if (r < a.n_rec) {
        const int64_t off = a.rec_off[r] - a.row_base, len = a.rec_len[r];
        bad = !bg_inside(off, len, a.n_pos);
        if (!bad && r > 0) {                                 // after the previous record and its separator
            const int64_t poff = a.rec_off[r - 1] - a.row_base, plen = a.rec_len[r - 1];
            bad = !bg_inside(poff, plen, a.n_pos) || off <= poff + plen;
        }
        double x[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) x[c] = 0.0;
        if (!bad) {
            const int64_t np = (len + BG_PIECE - 1) / BG_PIECE, slot0 = off / BG_PIECE + r;
            for (int64_t p = 0; p < np && slot0 + p < a.n_slots; ++p) {
                const double *q = part + (slot0 + p) * 7;
#pragma unroll
                for (int c = 0; c < 7; ++c) x[c] = p == 0 ? q[c] : x[c] + q[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) sums[r * 7 + c] = x[c];
    }
    const int64_t m = bg_block_min(bad ? r : BG_NONE, sh);
    if (threadIdx.x == 0) blk[blockIdx.x] = m;
}

// verdict[0] = the smallest bad flat element index, verdict[1] = the first record whose table entry is wrong
__global__ __launch_bounds__(BG_VERDICT_BLOCK) void k_bg_verdict(const int64_t *__restrict__ blk_cells, int64_t n_cells,
                                                                const int64_t *__restrict__ blk_recs, int64_t n_recs,
                                                                int64_t *__restrict__ verdict)
{
    __shared__ int64_t sh[BG_VERDICT_BLOCK];
    int64_t m = BG_NONE;
    for (int64_t i = threadIdx.x; i < n_cells; i += BG_VERDICT_BLOCK) m = min(m, blk_cells[i]);
    m = bg_block_min(m, sh);
    if (threadIdx.x == 0) verdict[0] = m;
    __syncthreads();
    m = BG_NONE;
    for (int64_t i = threadIdx.x; i < n_recs; i += BG_VERDICT_BLOCK) m = min(m, blk_recs[i]);
    m = bg_block_min(m, sh);
    if (threadIdx.x == 0) verdict[1] = m;
}

int bg_dtype(pfmscan_ctx *ctx, int dtype)
{
    if (dtype != PFMSCAN_PROFILE_F32 && dtype != PFMSCAN_PROFILE_F64)
        return fail(ctx, PFMSCAN_E_BADARG, "column sums: profile_dtype must be PFMSCAN_PROFILE_F32 or F64");
    return PFMSCAN_OK;
}

int64_t bg_slots(int64_t n_pos, int64_t n_rec) { return n_pos / BG_PIECE + n_rec; }
int64_t bg_rec_blocks(int64_t n_rec) { return (n_rec + BG_REC_BLOCK - 1) / BG_REC_BLOCK; }
// device scratch of one launch set: piece sums, per-workgroup keys of both kernels
size_t bg_part_bytes(int64_t n_pos, int64_t n_rec) { return (size_t)bg_slots(n_pos, n_rec) * 7 * sizeof(double); }
size_t bg_blk_words(int64_t n_pos, int64_t n_rec) { return (size_t)(bg_slots(n_pos, n_rec) + bg_rec_blocks(n_rec)); }

// Launches of one stream piece on `st`: sums of records [0, n_rec) of `a` into d_sums, the verdict into d_verdict[0..1].
// part / blk are scratch of at least bg_part_bytes / bg_blk_words.  Asynchronous.
int bg_launch(pfmscan_ctx *ctx, BgArgs a, int dtype, double *d_sums, double *part, int64_t *blk, int64_t *d_verdict,
              hipStream_t st)
{
    a.n_slots = bg_slots(a.n_pos, a.n_rec);
    const int64_t nb_rec = bg_rec_blocks(a.n_rec);
    if (a.n_slots > INT_MAX || nb_rec > INT_MAX) return fail(ctx, PFMSCAN_E_BADSHAPE, "column sums: too many pieces for one launch");
    if (a.n_slots > 0) {
        if (dtype == PFMSCAN_PROFILE_F64)
            hipLaunchKernelGGL(k_bg_pieces<double>, dim3((unsigned)a.n_slots), dim3(BG_BLOCK), 0, st, a, part, blk);
        else
            hipLaunchKernelGGL(k_bg_pieces<float>, dim3((unsigned)a.n_slots), dim3(BG_BLOCK), 0, st, a, part, blk);
    }
    hipLaunchKernelGGL(k_bg_records, dim3((unsigned)nb_rec), dim3(BG_REC_BLOCK), 0, st, a, part, d_sums, blk + a.n_slots);
    hipLaunchKernelGGL(k_bg_verdict, dim3(1), dim3(BG_VERDICT_BLOCK), 0, st, blk, a.n_slots, blk + a.n_slots, nb_rec, d_verdict);
    HIP_TRY(ctx, hipGetLastError());
    return PFMSCAN_OK;
}

// v[0..1] as k_bg_verdict wrote them -> status; cell_base is added to the reported element index
int bg_verdict(pfmscan_ctx *ctx, const int64_t *v, int64_t cell_base, int64_t rec_base, int64_t *first_bad)
{
    if (v[1] != BG_NONE)
        return fail(ctx, PFMSCAN_E_BADARG, "column sums: record " + std::to_string(rec_base + v[1]) +
                                               " lies outside the stream or does not follow the record before it");
    if (v[0] != BG_NONE) {
        const int64_t at = cell_base + v[0];
        if (first_bad) *first_bad = at;
        return fail(ctx, PFMSCAN_E_BADARG, "column sums: row " + std::to_string(at / 7) + ", column " + std::to_string(at % 7) +
                                               " is NaN, infinite or negative");
    }
    return PFMSCAN_OK;
}

int bg_dev(pfmscan_ctx *ctx, const void *d_profile, int dtype, int64_t n_pos, const int64_t *d_rec_off,
           const int64_t *d_rec_len, int64_t n_rec, double *d_sums, int64_t *first_bad, hipStream_t st)
{
    int rc = bg_dtype(ctx, dtype);
    if (rc) return rc;
    if (n_pos < 0 || n_rec < 0) return fail(ctx, PFMSCAN_E_BADARG, "column sums: negative size");
    if (n_rec == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || !d_sums || (n_pos > 0 && !d_profile)) return fail(ctx, PFMSCAN_E_BADARG, "column sums: NULL buffer");
    if (misaligned(d_profile)) return fail(ctx, PFMSCAN_E_BADSHAPE, "column sums: the profile must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->bg_part, bg_part_bytes(n_pos, n_rec) + 16))) return rc;
    if ((rc = ensure(ctx, ctx->bg_blk, (bg_blk_words(n_pos, n_rec) + 2) * sizeof(int64_t)))) return rc;
    int64_t *blk = static_cast<int64_t *>(ctx->bg_blk.p);
    int64_t *verdict = blk + bg_blk_words(n_pos, n_rec);
    BgArgs a;
    a.profile = static_cast<const unsigned char *>(d_profile);
    a.n_pos = n_pos;
    a.rec_off = d_rec_off;
    a.rec_len = d_rec_len;
    a.n_rec = n_rec;
    a.row_base = 0;
    a.n_slots = 0;
    if ((rc = bg_launch(ctx, a, dtype, d_sums, static_cast<double *>(ctx->bg_part.p), blk, verdict, st))) return rc;
    int64_t v[2] = {BG_NONE, BG_NONE};
    HIP_TRY(ctx, hipMemcpyAsync(v, verdict, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return bg_verdict(ctx, v, 0, 0, first_bad);
}

// host tables -> the ctx's device copy (rec_off at [0, n_rec), rec_len at [n_rec, 2 n_rec)) on the ctx's stream
int bg_upload_tables(pfmscan_ctx *ctx, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec)
{
    int rc = ensure(ctx, ctx->bg_tab, (size_t)n_rec * 2 * sizeof(int64_t));
    if (rc) return rc;
    int64_t *d = static_cast<int64_t *>(ctx->bg_tab.p);
    if ((rc = upload(ctx, d, rec_off, (size_t)n_rec * 8, ctx->stream))) return rc;
    return upload(ctx, d + n_rec, rec_len, (size_t)n_rec * 8, ctx->stream);
}

}  // namespace

extern "C" {

int pfmscan_profile_colsums_dev(pfmscan_ctx *ctx, const void *d_profile, int profile_dtype, int64_t n_pos,
                                const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_sums,
                                int64_t *first_bad, void *stream)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    return bg_dev(ctx, d_profile, profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec, d_sums, first_bad,
                  stream ? (hipStream_t)stream : ctx->stream);
}

int pfmscan_profile_colsums_staged(pfmscan_ctx *ctx, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec,
                                   double *sums, int64_t *first_bad)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    if (ctx->staged_n < 0 || !ctx->staged_profile) return fail(ctx, PFMSCAN_E_BADARG, "column sums: no profile is staged");
    if (n_rec < 0) return fail(ctx, PFMSCAN_E_BADARG, "column sums: negative size");
    if (n_rec == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len || !sums) return fail(ctx, PFMSCAN_E_BADARG, "column sums: NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bg_upload_tables(ctx, rec_off, rec_len, n_rec);
    if (rc) return rc;
    if ((rc = ensure(ctx, ctx->bg_sums, (size_t)n_rec * 7 * sizeof(double)))) return rc;
    const int64_t *d = static_cast<const int64_t *>(ctx->bg_tab.p);
    rc = bg_dev(ctx, ctx->profile.p, ctx->staged_dtype, ctx->staged_n, d, d + n_rec, n_rec, static_cast<double *>(ctx->bg_sums.p),
                first_bad, ctx->stream);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(sums, ctx->bg_sums.p, (size_t)n_rec * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFMSCAN_OK;
}

int pfmscan_profile_colsums_host(pfmscan_ctx *ctx, const void *profile, int profile_dtype, int64_t n_pos,
                                 const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *sums,
                                 int64_t *first_bad)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    int rc = bg_dtype(ctx, profile_dtype);
    if (rc) return rc;
    if (n_pos < 0 || n_rec < 0) return fail(ctx, PFMSCAN_E_BADARG, "column sums: negative size");
    if (n_rec == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len || !sums || (n_pos > 0 && !profile)) return fail(ctx, PFMSCAN_E_BADARG, "column sums: NULL argument");
    // the table is checked here: the cuts below rely on it (the device checks it again for the _dev form)
    for (int64_t r = 0; r < n_rec; ++r) {
        const bool inside = rec_off[r] >= 0 && rec_len[r] >= 0 && rec_off[r] <= n_pos && rec_len[r] <= n_pos - rec_off[r];
        if (!inside || (r > 0 && rec_off[r] <= rec_off[r - 1] + rec_len[r - 1]))
            return fail(ctx, PFMSCAN_E_BADARG, "column sums: record " + std::to_string(r) +
                                                   " lies outside the stream or does not follow the record before it");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t row_bytes = (size_t)7 * (profile_dtype == PFMSCAN_PROFILE_F32 ? 4 : 8);
    // pieces of whole records, at most `chunk` rows each (a longer record is a piece of its own): [r0, r1) per piece
    int64_t chunk = (int64_t)1 << 24;
    if (const char *e = std::getenv("PFMSCAN_COLSUMS_CHUNK")) chunk = std::max<int64_t>(1, std::atoll(e));
    std::vector<int64_t> cuts(1, 0);
    int64_t max_rows = 0, max_rec = 0;
    for (int64_t r = 0; r < n_rec;) {
        const int64_t first = rec_off[r];
        int64_t e = r + 1;
        while (e < n_rec && rec_off[e] + rec_len[e] - first <= chunk) ++e;
        max_rows = std::max(max_rows, rec_off[e - 1] + rec_len[e - 1] - first);
        max_rec = std::max(max_rec, e - r);
        cuts.push_back(e);
        r = e;
    }
    const int64_t n_cuts = (int64_t)cuts.size() - 1;
    if ((rc = bg_upload_tables(ctx, rec_off, rec_len, n_rec))) return rc;
    if ((rc = ensure(ctx, ctx->bg_sums, (size_t)n_rec * 7 * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->bg_part, bg_part_bytes(max_rows, max_rec) + 16))) return rc;
    const size_t blk_words = bg_blk_words(max_rows, max_rec);
    if ((rc = ensure(ctx, ctx->bg_blk, (blk_words + 2 * (size_t)n_cuts) * sizeof(int64_t)))) return rc;
    if (!ctx->copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if ((rc = ensure(ctx, ctx->pipe_profile[i], std::max<size_t>((size_t)max_rows * row_bytes, 16)))) return rc;
        if (!ctx->pipe_copied[i]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe_copied[i], hipEventDisableTiming));
        if (!ctx->pipe_scanned[i]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe_scanned[i], hipEventDisableTiming));
    }
    const int64_t *d_tab = static_cast<const int64_t *>(ctx->bg_tab.p);
    double *d_sums = static_cast<double *>(ctx->bg_sums.p);
    int64_t *blk = static_cast<int64_t *>(ctx->bg_blk.p);
    int64_t *verdicts = blk + blk_words;
    // the tables are uploaded on the ctx's stream, which also runs every launch; the copy stream only moves rows
    auto rows_of = [&](int64_t k, int64_t *first) {
        const int64_t r0 = cuts[k], r1 = cuts[k + 1];
        *first = rec_off[r0];
        return rec_off[r1 - 1] + rec_len[r1 - 1] - rec_off[r0];
    };
    auto send = [&](int64_t k) -> int {
        const int b = (int)(k & 1);
        int64_t first = 0;
        const int64_t rows = rows_of(k, &first);
        if (k >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->pipe_scanned[b], 0));
        if (rows > 0)
            if (int urc = upload(ctx, ctx->pipe_profile[b].p, static_cast<const unsigned char *>(profile) + (size_t)first * row_bytes,
                                 (size_t)rows * row_bytes, ctx->copy_stream))
                return urc;
        HIP_TRY(ctx, hipEventRecord(ctx->pipe_copied[b], ctx->copy_stream));
        return PFMSCAN_OK;
    };
    if ((rc = send(0))) return rc;
    for (int64_t k = 0; k < n_cuts; ++k) {
        const int b = (int)(k & 1);
        int64_t first = 0;
        const int64_t rows = rows_of(k, &first);
        const int64_t r0 = cuts[k], r1 = cuts[k + 1];
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->pipe_copied[b], 0));
        BgArgs a;
        a.profile = static_cast<const unsigned char *>(ctx->pipe_profile[b].p);
        a.n_pos = rows;
        a.rec_off = d_tab + r0;
        a.rec_len = d_tab + n_rec + r0;
        a.n_rec = r1 - r0;
        a.row_base = first;
        a.n_slots = 0;
        if ((rc = bg_launch(ctx, a, profile_dtype, d_sums + r0 * 7, static_cast<double *>(ctx->bg_part.p), blk, verdicts + 2 * k,
                            ctx->stream)))
            return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->pipe_scanned[b], ctx->stream));
        if (k + 1 < n_cuts && (rc = send(k + 1))) return rc;
    }
    std::vector<int64_t> v((size_t)n_cuts * 2, BG_NONE);
    HIP_TRY(ctx, hipMemcpyAsync(v.data(), verdicts, v.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t k = 0; k < n_cuts; ++k)                     // pieces are in input order: the first rejected one holds the earliest cell
        if ((rc = bg_verdict(ctx, &v[(size_t)k * 2], rec_off[cuts[k]] * 7, cuts[k], first_bad))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, (size_t)n_rec * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFMSCAN_OK;
}

}  // extern "C"
