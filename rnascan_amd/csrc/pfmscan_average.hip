// pfmscan_average.hip -- per-fragment structure letters -> averaged-structure profile rows on the device.
//
// Replaces the counting half of rnascan/average_structure.py (get_structure_probability_matrix_for_sequence, :44-99:
// align the annotated fragments with '-' gaps, :89-92; count B E H L M R T per position, struct_pfm_from_aligned :28-42;
// divide by the position's total, norm_pfm in pfmutil.py:136-151) for every record of a batch at once.  The folding that
// produces the fragments' structures stays outside (RNAfold); the annotation is pfmscan_dotbracket.hip.
//
//   k_avg_check   one lane per record: the record and fragment tables are consistent (contiguous rows, sorted starts,
//                 fragments inside their record and inside the letter stream, no fragment longer than max_len)
//   k_avg_rows    OUTPUT-STATIONARY: one lane owns one output row; a wave owns AVG_TILE consecutive rows.  The wave walks
//                 the fragments that can reach its rows (starts in (row0 - max_len, row0 + AVG_TILE), found by a binary
//                 search over the sorted starts) and every lane reads the one letter of the fragment at its row: lanes
//                 read consecutive bytes, every fragment byte is read once in all.  Counts are packed 16-bit fields in
//                 two 64-bit words (no register array); the row is then T[n(n+1)/2 + c] per column -- the value the scan
//                 would read back from the reference's text -- and written through LDS as contiguous wave stores.
//   k_avg_verdict one workgroup: the smallest error key over the per-workgroup keys of both kernels.
//
// No global atomics: errors are per-workgroup minima, reduced by a separate launch.  Every load is bounded (stream,
// tables, T) whatever the input, so k_avg_rows may run before the host has read k_avg_check's verdict.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>
#include <cstring>
#include <string>

#include "pfmscan_ctx.hpp"

using namespace pfmscan;

namespace {

constexpr int AVG_TILE = 64;                     // rows per wave (one per lane)
constexpr int AVG_WAVES = 4;
constexpr int AVG_BLOCK = AVG_TILE * AVG_WAVES;
constexpr int AVG_CHECK_BLOCK = 256;
constexpr int AVG_VERDICT_BLOCK = 1024;
constexpr int64_t AVG_NONE = INT64_MAX;

// error keys: (index << 2) | kind, the smallest one wins
enum : int64_t { K_UNCOVERED = 0, K_COVER = 1, K_TABLE = 2 };

struct AvgTables {
    const uint8_t *letters;
    int64_t n_letters;
    const int64_t *frag_off, *frag_len, *frag_row;
    int64_t n_frag, max_len;
    const int64_t *rec_row, *rec_len, *rec_frag;     // rec_frag [n_rec + 1]
    int64_t n_rec, n_rows;
};

__device__ inline int64_t block_min(int64_t v, int64_t *sh)
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

__global__ __launch_bounds__(AVG_CHECK_BLOCK) void k_avg_check(AvgTables a, int64_t *__restrict__ blk)
{
    __shared__ int64_t sh[AVG_CHECK_BLOCK];
    const int64_t r = (int64_t)blockIdx.x * AVG_CHECK_BLOCK + threadIdx.x;
    bool bad = false;
    if (r < a.n_rec) {
        const int64_t row = a.rec_row[r], len = a.rec_len[r];
        const int64_t f0 = a.rec_frag[r], f1 = a.rec_frag[r + 1];
        const int64_t want_row = r == 0 ? 0 : a.rec_row[r - 1] + a.rec_len[r - 1] + 1;
        bad = len < 0 || row != want_row || f0 < 0 || f1 < f0 || f1 > a.n_frag || (r == 0 && f0 != 0) ||
              (r == a.n_rec - 1 && (f1 != a.n_frag || row + len + 1 != a.n_rows));
        if (!bad) {
            int64_t prev = row;
            for (int64_t f = f0; f < f1 && !bad; ++f) {
                const int64_t s = a.frag_row[f], n = a.frag_len[f], o = a.frag_off[f];
                bad = s < prev || n < 1 || n > a.max_len || s + n > row + len || o < 0 || o > a.n_letters - n;
                prev = s;
            }
        }
    }
    const int64_t m = block_min(bad ? (r << 2 | K_TABLE) : AVG_NONE, sh);
    if (threadIdx.x == 0) blk[blockIdx.x] = m;
}

// first index in [lo, hi) whose frag_row exceeds `key` (hi when none); wave-uniform arguments
__device__ inline int64_t first_above(const int64_t *__restrict__ rows, int64_t lo, int64_t hi, int64_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (rows[mid] > key) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

template <typename OUT>
__global__ __launch_bounds__(AVG_BLOCK) void k_avg_rows(AvgTables a, const double *__restrict__ T, int64_t n_T, int n_max,
                                                       OUT *__restrict__ out, int64_t *__restrict__ blk)
{
    __shared__ int64_t sh[AVG_BLOCK];
    __shared__ OUT stage[AVG_WAVES][AVG_TILE * 7];
    const int lane = threadIdx.x % AVG_TILE, wave = threadIdx.x / AVG_TILE;
    const int64_t row0 = ((int64_t)blockIdx.x * AVG_WAVES + wave) * AVG_TILE;
    const int64_t row = row0 + lane;
    int64_t key = AVG_NONE;
    double v[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = 0.0;
    if (row0 < a.n_rows) {                       // wave-uniform
        // the record holding row0: the last r with rec_row[r] <= row0
        int64_t lo = 0, hi = a.n_rec;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.rec_row[mid] <= row0) lo = mid;
            else hi = mid;
        }
        uint64_t c_lo = 0, c_hi = 0;             // 16-bit counts: B E H L | M R T
        int n = 0;
        bool sep = false;
        const int64_t last = row0 + AVG_TILE - 1;
        for (int64_t r = lo; r < a.n_rec; ++r) {
            const int64_t rr = a.rec_row[r];
            if (rr > last) break;
            if (row == rr + a.rec_len[r]) sep = true;
            const int64_t f1 = min(max(a.rec_frag[r + 1], (int64_t)0), a.n_frag);
            int64_t f = min(max(a.rec_frag[r], (int64_t)0), f1);
            f = first_above(a.frag_row, f, f1, row0 - a.max_len);
            for (; f < f1; ++f) {
                const int64_t s = a.frag_row[f];
                if (s > last) break;
                const int64_t q = row - s;
                const int64_t fl = a.frag_len[f], fo = a.frag_off[f];
                if (q >= 0 && q < fl && fo + q >= 0 && fo + q < a.n_letters) {
                    const uint32_t c = a.letters[fo + q];
                    c_lo += c < 4 ? (uint64_t)1 << (16 * c) : 0;
                    c_hi += (c >= 4 && c < 7) ? (uint64_t)1 << (16 * (c - 4)) : 0;
                    n += c < 7;
                }
            }
        }
        if (row < a.n_rows && !sep) {
            if (n == 0 || n > n_max) {
                key = row << 2 | (n == 0 ? K_UNCOVERED : K_COVER);
            } else {
                const int64_t base = (int64_t)n * (n + 1) / 2;
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const int64_t c = (int64_t)((k < 4 ? c_lo >> (16 * k) : c_hi >> (16 * (k - 4))) & 0xffff);
                    const int64_t i = base + c;
                    v[k] = i < n_T ? T[i] : 0.0;
                }
            }
        }
    }
    // through LDS: each wave then stores its rows as one contiguous range, 64 consecutive elements per store
    OUT *st = stage[wave];
#pragma unroll
    for (int k = 0; k < 7; ++k) st[lane * 7 + k] = (OUT)v[k];
    __syncthreads();
    if (row0 < a.n_rows) {
        const int64_t valid = min((int64_t)AVG_TILE, a.n_rows - row0) * 7;
        OUT *dst = out + row0 * 7;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int e = j * AVG_TILE + lane;
            if (e < valid) dst[e] = st[e];
        }
    }
    const int64_t m = block_min(key, sh);
    if (threadIdx.x == 0) blk[blockIdx.x] = m;
}

// blk[0, n_check) are k_avg_check's keys (records), blk[n_check, n) k_avg_rows' (rows).  A record index and a row index do not
// compare: rows computed from a broken table mean nothing, so the earliest broken record wins over every row (record 0 with
// its row 0 left uncovered by a fragment of length 0 used to come out as AVG_UNCOVERED at row 0).
__global__ __launch_bounds__(AVG_VERDICT_BLOCK) void k_avg_verdict(const int64_t *__restrict__ blk, int64_t n_check, int64_t n,
                                                                   int64_t *__restrict__ verdict)
{
    __shared__ int64_t sh[AVG_VERDICT_BLOCK];
    int64_t mt = AVG_NONE, mr = AVG_NONE;
    for (int64_t i = threadIdx.x; i < n; i += AVG_VERDICT_BLOCK) {
        if (i < n_check) mt = min(mt, blk[i]);
        else mr = min(mr, blk[i]);
    }
    mt = block_min(mt, sh);
    __syncthreads();
    mr = block_min(mr, sh);
    if (threadIdx.x == 0) verdict[0] = mt != AVG_NONE ? mt : mr;
}

// E H T B L R M (the annotation's letter order) -> their columns in B E H L M R T (write_pfm's sorted order)
const uint8_t ANNOTATE_MAP[7] = {1, 2, 6, 0, 3, 5, 4};

int check_dtype(pfmscan_ctx *ctx, int dtype)
{
    if (dtype != PFMSCAN_PROFILE_F32 && dtype != PFMSCAN_PROFILE_F64)
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: out_dtype must be PFMSCAN_PROFILE_F32 or F64");
    return PFMSCAN_OK;
}

// the rows of every record on `st`; synchronises `st` once for the verdict.  *first_bad / *bad_kind as in the header.
int average_rows(pfmscan_ctx *ctx, const AvgTables &a, const double *d_T, int n_max, void *d_out, int dtype,
                 int64_t *first_bad, int *bad_kind, hipStream_t st)
{
    if (first_bad) *first_bad = -1;
    if (bad_kind) *bad_kind = PFMSCAN_AVG_OK;
    int rc = check_dtype(ctx, dtype);
    if (rc) return rc;
    if (a.n_rec < 0 || a.n_frag < 0 || a.n_letters < 0 || a.n_rows < 0)
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: negative size");
    if (n_max < 0 || n_max > PFMSCAN_MAX_COVER)
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: n_max must be 0.." + std::to_string(PFMSCAN_MAX_COVER));
    if (a.n_rec == 0) {
        if (a.n_rows != 0 || a.n_frag != 0) return fail(ctx, PFMSCAN_E_BADARG, "averaging: rows or fragments without records");
        return PFMSCAN_OK;
    }
    if (!a.rec_row || !a.rec_len || !a.rec_frag || !d_out || !d_T || (a.n_frag > 0 && (!a.frag_off || !a.frag_len || !a.frag_row || !a.letters)))
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: NULL buffer");
    if (a.max_len < 1 && a.n_frag > 0) return fail(ctx, PFMSCAN_E_BADARG, "averaging: max_len must be >= 1");
    const int64_t n_T = (int64_t)(n_max + 1) * (n_max + 2) / 2;
    const int64_t nb_check = (a.n_rec + AVG_CHECK_BLOCK - 1) / AVG_CHECK_BLOCK;
    const int64_t nb_rows = (a.n_rows + AVG_BLOCK - 1) / AVG_BLOCK;
    if (nb_check > INT_MAX || nb_rows > INT_MAX) return fail(ctx, PFMSCAN_E_BADSHAPE, "averaging: too many rows");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->avg_blk, (size_t)(nb_check + nb_rows + 1) * sizeof(int64_t)))) return rc;
    int64_t *blk = static_cast<int64_t *>(ctx->avg_blk.p);
    int64_t *verdict = blk + nb_check + nb_rows;
    hipLaunchKernelGGL(k_avg_check, dim3((unsigned)nb_check), dim3(AVG_CHECK_BLOCK), 0, st, a, blk);
    if (nb_rows > 0) {
        if (dtype == PFMSCAN_PROFILE_F64)
            hipLaunchKernelGGL(k_avg_rows<double>, dim3((unsigned)nb_rows), dim3(AVG_BLOCK), 0, st, a, d_T, n_T, n_max,
                               static_cast<double *>(d_out), blk + nb_check);
        else
            hipLaunchKernelGGL(k_avg_rows<float>, dim3((unsigned)nb_rows), dim3(AVG_BLOCK), 0, st, a, d_T, n_T, n_max,
                               static_cast<float *>(d_out), blk + nb_check);
    }
    hipLaunchKernelGGL(k_avg_verdict, dim3(1), dim3(AVG_VERDICT_BLOCK), 0, st, blk, nb_check, nb_check + nb_rows, verdict);
    HIP_TRY(ctx, hipGetLastError());
    int64_t v = AVG_NONE;
    HIP_TRY(ctx, hipMemcpyAsync(&v, verdict, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (v == AVG_NONE) return PFMSCAN_OK;
    const int64_t at = v >> 2, kind = v & 3;
    if (first_bad) *first_bad = at;
    if (kind == K_TABLE) {
        if (bad_kind) *bad_kind = PFMSCAN_AVG_BAD_TABLE;
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: inconsistent record / fragment table at record " + std::to_string(at));
    }
    if (kind == K_UNCOVERED) {
        if (bad_kind) *bad_kind = PFMSCAN_AVG_UNCOVERED;
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: no fragment covers row " + std::to_string(at));
    }
    if (bad_kind) *bad_kind = PFMSCAN_AVG_COVER;
    return fail(ctx, PFMSCAN_E_BADSHAPE, "averaging: row " + std::to_string(at) + " is covered by more than " +
                                             std::to_string(n_max) + " fragments");
}

// host tables + host dot-bracket codes -> annotated letters and rows in the ctx's scratch; rows land in `rows`
int average_from_host(pfmscan_ctx *ctx, const uint8_t *codes, int64_t n_pos, const int64_t *frag_off, const int64_t *frag_len,
                      const int64_t *frag_row, int64_t n_frag, const int64_t *rec_row, const int64_t *rec_len,
                      const int64_t *rec_frag, int64_t n_rec, const double *table, int n_max, int dtype, DevBuf &rows,
                      int64_t *n_rows_out, int64_t *first_bad, int *bad_kind)
{
    if (first_bad) *first_bad = -1;
    if (bad_kind) *bad_kind = PFMSCAN_AVG_OK;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    int rc = check_dtype(ctx, dtype);
    if (rc) return rc;
    if (n_pos < 0 || n_frag < 0 || n_rec < 0) return fail(ctx, PFMSCAN_E_BADARG, "averaging: negative size");
    if ((n_pos > 0 && !codes) || (n_frag > 0 && (!frag_off || !frag_len || !frag_row)) ||
        (n_rec > 0 && (!rec_row || !rec_len || !rec_frag)) || !table)
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: NULL argument");
    if (n_max < 0 || n_max > PFMSCAN_MAX_COVER)
        return fail(ctx, PFMSCAN_E_BADARG, "averaging: n_max must be 0.." + std::to_string(PFMSCAN_MAX_COVER));
    int64_t max_len = 1, n_rows = 0;
    for (int64_t f = 0; f < n_frag; ++f) max_len = frag_len[f] > max_len ? frag_len[f] : max_len;
    for (int64_t r = 0; r < n_rec; ++r) n_rows += rec_len[r] + 1;
    *n_rows_out = n_rows;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n_T = (int64_t)(n_max + 1) * (n_max + 2) / 2;
    const size_t tab_bytes = (size_t)(3 * n_frag + 3 * n_rec + 1) * sizeof(int64_t) + (size_t)n_T * sizeof(double);
    const size_t row_bytes = (size_t)n_rows * 7 * (dtype == PFMSCAN_PROFILE_F32 ? 4 : 8);
    if ((rc = ensure(ctx, ctx->avg_tab, tab_bytes))) return rc;
    if ((rc = ensure(ctx, rows, row_bytes > 0 ? row_bytes : 16))) return rc;
    if (n_pos > 0) {
        if ((rc = ensure(ctx, ctx->db_in, (size_t)n_pos))) return rc;
        if ((rc = ensure(ctx, ctx->db_out, (size_t)n_pos))) return rc;
        if ((rc = upload(ctx, ctx->db_in.p, codes, (size_t)n_pos, ctx->stream))) return rc;
    }
    double *d_T = static_cast<double *>(ctx->avg_tab.p);
    int64_t *t64 = reinterpret_cast<int64_t *>(d_T + n_T);
    struct Piece { const void *src; size_t bytes; void *dst; };
    const Piece pieces[] = {{table, (size_t)n_T * sizeof(double), d_T},
                            {frag_off, (size_t)n_frag * 8, t64},
                            {frag_len, (size_t)n_frag * 8, t64 + n_frag},
                            {frag_row, (size_t)n_frag * 8, t64 + 2 * n_frag},
                            {rec_row, (size_t)n_rec * 8, t64 + 3 * n_frag},
                            {rec_len, (size_t)n_rec * 8, t64 + 3 * n_frag + n_rec},
                            {rec_frag, (size_t)(n_rec > 0 ? n_rec + 1 : 0) * 8, t64 + 3 * n_frag + 2 * n_rec}};
    for (const Piece &p : pieces)
        if (p.bytes && (rc = upload(ctx, p.dst, p.src, p.bytes, ctx->stream))) return rc;
    int64_t bad = -1;
    int64_t counts[7];
    rc = dotbracket_annotate(ctx, static_cast<const uint8_t *>(ctx->db_in.p), static_cast<uint8_t *>(ctx->db_out.p), n_pos,
                             ANNOTATE_MAP, nullptr, counts, &bad, ctx->stream);
    if (rc) {
        if (bad >= 0) {
            if (first_bad) *first_bad = bad;
            if (bad_kind) *bad_kind = PFMSCAN_AVG_DOTBRACKET;
        }
        return rc;
    }
    AvgTables a;
    a.letters = static_cast<const uint8_t *>(ctx->db_out.p);
    a.n_letters = n_pos;
    a.frag_off = t64;
    a.frag_len = t64 + n_frag;
    a.frag_row = t64 + 2 * n_frag;
    a.n_frag = n_frag;
    a.max_len = max_len;
    a.rec_row = t64 + 3 * n_frag;
    a.rec_len = t64 + 3 * n_frag + n_rec;
    a.rec_frag = t64 + 3 * n_frag + 2 * n_rec;
    a.n_rec = n_rec;
    a.n_rows = n_rows;
    return average_rows(ctx, a, d_T, n_max, rows.p, dtype, first_bad, bad_kind, ctx->stream);
}

}  // namespace

extern "C" {

int pfmscan_average_dev(pfmscan_ctx *ctx, const uint8_t *d_letters, int64_t n_letters, const int64_t *d_frag_off,
                        const int64_t *d_frag_len, const int64_t *d_frag_row, int64_t n_frag, int64_t max_len,
                        const int64_t *d_rec_row, const int64_t *d_rec_len, const int64_t *d_rec_frag, int64_t n_rec,
                        int64_t n_rows, const double *d_table, int n_max, void *d_out, int out_dtype, int64_t *first_bad,
                        int *bad_kind, void *stream)
{
    if (first_bad) *first_bad = -1;
    if (bad_kind) *bad_kind = PFMSCAN_AVG_OK;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    AvgTables a;
    a.letters = d_letters;
    a.n_letters = n_letters;
    a.frag_off = d_frag_off;
    a.frag_len = d_frag_len;
    a.frag_row = d_frag_row;
    a.n_frag = n_frag;
    a.max_len = max_len;
    a.rec_row = d_rec_row;
    a.rec_len = d_rec_len;
    a.rec_frag = d_rec_frag;
    a.n_rec = n_rec;
    a.n_rows = n_rows;
    return average_rows(ctx, a, d_table, n_max, d_out, out_dtype, first_bad, bad_kind, stream ? (hipStream_t)stream : ctx->stream);
}

int pfmscan_average_host(pfmscan_ctx *ctx, const uint8_t *codes, int64_t n_pos, const int64_t *frag_off,
                         const int64_t *frag_len, const int64_t *frag_row, int64_t n_frag, const int64_t *rec_row,
                         const int64_t *rec_len, const int64_t *rec_frag, int64_t n_rec, const double *table, int n_max,
                         void *out, int out_dtype, int64_t *first_bad, int *bad_kind)
{
    if (first_bad) *first_bad = -1;
    if (bad_kind) *bad_kind = PFMSCAN_AVG_OK;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    int64_t n_rows = 0;
    int rc = average_from_host(ctx, codes, n_pos, frag_off, frag_len, frag_row, n_frag, rec_row, rec_len, rec_frag, n_rec,
                               table, n_max, out_dtype, ctx->avg_out, &n_rows, first_bad, bad_kind);
    if (rc) return rc;
    if (n_rows > 0) {
        if (!out) return fail(ctx, PFMSCAN_E_BADARG, "averaging: NULL out");
        const size_t bytes = (size_t)n_rows * 7 * (out_dtype == PFMSCAN_PROFILE_F32 ? 4 : 8);
        HIP_TRY(ctx, hipMemcpyAsync(out, ctx->avg_out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PFMSCAN_OK;
}

int pfmscan_average_stage(pfmscan_ctx *ctx, const uint8_t *codes, int64_t n_pos, const int64_t *frag_off,
                          const int64_t *frag_len, const int64_t *frag_row, int64_t n_frag, const int64_t *rec_row,
                          const int64_t *rec_len, const int64_t *rec_frag, int64_t n_rec, const double *table, int n_max,
                          int out_dtype, int64_t *n_rows, int64_t *first_bad, int *bad_kind)
{
    if (first_bad) *first_bad = -1;
    if (bad_kind) *bad_kind = PFMSCAN_AVG_OK;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    ctx->staged_n = -1;
    int64_t rows = 0;
    int rc = average_from_host(ctx, codes, n_pos, frag_off, frag_len, frag_row, n_frag, rec_row, rec_len, rec_frag, n_rec,
                               table, n_max, out_dtype, ctx->profile, &rows, first_bad, bad_kind);
    if (rc) return rc;
    if (n_rows) *n_rows = rows;
    ctx->staged_n = rows;
    ++ctx->stage_serial;
    ctx->staged_dtype = out_dtype;
    ctx->staged_codes = false;
    ctx->staged_profile = true;
    ctx->staged_codes2 = false;
    return PFMSCAN_OK;
}

int pfmscan_fragment_ids(const uint8_t *buf, const int64_t *id_off, const int64_t *id_len, int64_t n, int64_t *key_len,
                         int64_t *start, int64_t *first_bad)
{
    static const char TAG[] = "_frag_";
    const int64_t tag = 6;
    if (first_bad) *first_bad = -1;
    if (n < 0) return fail(nullptr, PFMSCAN_E_BADARG, "negative n");
    if (n > 0 && (!buf || !id_off || !id_len || !key_len || !start))
        return fail(nullptr, PFMSCAN_E_BADARG, "NULL argument");
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t *s = buf + id_off[i];
        const int64_t len = id_len[i];
        int64_t at = -1;
        for (int64_t j = len - tag; j >= 1; --j)            // the LAST "_frag_", after a key of at least one byte
            if (std::memcmp(s + j, TAG, tag) == 0) {
                at = j;
                break;
            }
        bool ok = at > 0;
        int64_t v = 0;
        if (ok) {
            int64_t p = at + tag;
            const bool neg = p < len && s[p] == '-';
            p += neg;
            ok = p < len && len - p <= 18;
            for (; ok && p < len; ++p) {
                ok = s[p] >= '0' && s[p] <= '9';
                v = v * 10 + (s[p] - '0');
            }
            v = neg ? -v : v;
        }
        if (!ok) {
            if (first_bad) *first_bad = i;
            return fail(nullptr, PFMSCAN_E_BADARG, "fragment id " + std::to_string(i) + " does not end in _frag_<start>");
        }
        key_len[i] = at;
        start[i] = v;
    }
    return PFMSCAN_OK;
}

}  // extern "C"
