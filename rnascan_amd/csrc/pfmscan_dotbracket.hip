// pfmscan_dotbracket.hip -- dot-bracket structures -> structure-context letters (EHTBLRM) on the device.
//
// Replaces scripts/parse_secondary_structure.cpp (parse(), :65-221, run one line at a time by its main(), :235-261):
// the reference pairs brackets with a forward scan per '(' (findPairs, :13-43) and tests every loop against every pair
// left of it, quadratic in the worst case.  Here the whole packed stream (include/pfmscan.h: one separator, code 7,
// after every record) is annotated in a few memory-bound launches:
//
//   k_db_tiles     per tile of DB_TILE positions: bracket balance, first / last non-dot, first / last separator
//   k_db_scan      ONE workgroup: exclusive scans over the tile summaries (depth before the tile, nearest non-dot left
//                  and right of it), and the check that no record is 2^31 positions or longer
//   k_db_depth     depth after every position (int32), the validity checks, the 64-ary min-tree's first two levels
//   k_db_level     the min-tree's upper levels (per 64^3, 64^4, ... positions), one small launch each
//   --- the host reads the verdict (first bad position); nothing below runs on an invalid stream ---
//   k_db_pairs     every '(' finds its partner: the first later position whose depth is smaller (a nearest-smaller-value
//                  query, answered by climbing the min-tree and descending it again); partners are int32 offsets
//   k_db_label<0>  loop labels of rule 2, and the multiloop marks of rule 3 (benign scatter of 1-bytes)
//   k_db_label<1>  the labels again, N -> M where the run was marked, else T; the caller's codes and the histogram
//
// No launch waits on another workgroup: every cross-tile dependency goes through a separate launch (reduce, scan,
// apply), so the result does not depend on dispatch order.  Every read is bounded by the stream's end, whatever the input.
//
// The rules (restated in tests/dotbracket_rules.py, pinned there against the reference binary's output):
//   '(' -> L, ')' -> R.  A maximal run of dots [a, b), k = a - 1, m = b:
//   k < 0 or m == n (the record's ends) -> E;  s[k] '(' and s[m] ')' -> H;  s[k] ')' and s[m] '(' -> M if depth(a) > 0,
//   else E;  s[k] == s[m] -> B if p[m] + 1 == p[k], else N.  For every ')' at j followed (at j + 1) by an L or an M,
//   with m the first bracket at or after j + 1: the N of the run ending at p[j] - 1 and of the run starting at
//   p[m] + 1 become M.  The remaining N become T.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <string>

#include "pfmscan_ctx.hpp"

using namespace pfmscan;

namespace {

constexpr int DB_BLOCK = 256;
constexpr int DB_PER = 16;                       // positions per thread (consecutive)
constexpr int DB_TILE = DB_BLOCK * DB_PER;       // 4096 positions per workgroup
constexpr int DB_SCAN_BLOCK = 1024;
constexpr int DB_MAXL = 8;                       // levels of the min-tree: 64^7 > 2^41 positions
constexpr int64_t DB_NONE = INT64_MAX;
constexpr int64_t DB_MAX_RECORD = (int64_t)1 << 31;

enum : uint8_t { C_DOT = 0, C_OPEN = 1, C_CLOSE = 2, C_OTHER = 3, C_SEP = PFMSCAN_SEP };
enum : int { L_E = 0, L_H = 1, L_T = 2, L_B = 3, L_L = 4, L_R = 5, L_M = 6, L_N = 7 };   // EHTBLRM + provisional N

struct TileArrays {
    int32_t *sum;            // '(' minus ')' in the tile
    int64_t *last_nd;        // last non-dot position in the tile (pos << 3 | code), -1: none
    int64_t *first_nd;       // first non-dot position (pos << 3 | code), DB_NONE: none
    int64_t *last_sep;       // last separator position, -1: none
    int64_t *first_sep;      // first separator position, DB_NONE: none
    int64_t *pre;            // k_db_scan: depth before the tile
    int64_t *prev_nd;        // k_db_scan: last non-dot before the tile (pos << 3 | code), -1: none
    int64_t *next_nd;        // k_db_scan: first non-dot after the tile (pos << 3 | code), DB_NONE: none
};

struct Tree {                // the 64-ary min-tree of depth: level 0 is the depth itself, level l + 1 the minima of 64 of level l
    int32_t *base;
    int64_t off[DB_MAXL];    // element offset of each level in base
    int64_t cnt[DB_MAXL];    // entries per level
    int nl;                  // levels in use; cnt[nl - 1] <= 64
};

struct Flags {               // device scratch: verdicts (min-reduced; memset to 0x7f.. = "none") and the histogram
    int64_t first_bad;
    int64_t first_long;
    int64_t counts[8];
};

__device__ inline void load16(const uint8_t *__restrict__ in, int64_t p0, int64_t n, uint8_t c[DB_PER])
{
    if (p0 + DB_PER <= n && ((reinterpret_cast<uintptr_t>(in + p0) & 15u) == 0)) {
        uint4 v = *reinterpret_cast<const uint4 *>(in + p0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < DB_PER; ++k) c[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < DB_PER; ++k) c[k] = (p0 + k < n) ? in[p0 + k] : (uint8_t)C_SEP;
    }
}

__device__ inline int delta_of(uint8_t c) { return c == C_OPEN ? 1 : (c == C_CLOSE ? -1 : 0); }

// inclusive scans over a workgroup of N threads: within each wave by lane shuffles, then across the N / 64 waves through
// `sh` (N / 64 entries) -- two barriers per scan
struct OpSum { __device__ int64_t operator()(int64_t a, int64_t b) const { return a + b; } };
struct OpMax { __device__ int64_t operator()(int64_t a, int64_t b) const { return max(a, b); } };
struct OpMin { __device__ int64_t operator()(int64_t a, int64_t b) const { return min(a, b); } };

template <int N, class Op>
__device__ int64_t scan_prefix(int64_t v, int64_t *sh, Op op)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up((long long)v, d);
        if (lane >= d) v = op(v, u);
    }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    for (int k = 0; k < w; ++k) v = op(v, sh[k]);
    __syncthreads();
    return v;
}
template <int N, class Op>   // suffix: thread t gets op over threads t .. N-1
__device__ int64_t scan_suffix(int64_t v, int64_t *sh, Op op)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_down((long long)v, d);
        if (lane + d < 64) v = op(v, u);
    }
    if (lane == 0) sh[w] = v;
    __syncthreads();
    for (int k = w + 1; k < N / 64; ++k) v = op(v, sh[k]);
    __syncthreads();
    return v;
}
template <int N> __device__ int64_t scan_sum(int64_t v, int64_t *sh) { return scan_prefix<N>(v, sh, OpSum()); }
template <int N> __device__ int64_t scan_max(int64_t v, int64_t *sh) { return scan_prefix<N>(v, sh, OpMax()); }
template <int N> __device__ int64_t scan_min_suffix(int64_t v, int64_t *sh) { return scan_suffix<N>(v, sh, OpMin()); }

__device__ inline int64_t block_min(int64_t v, int64_t *sh)
{
    v = scan_min_suffix<DB_BLOCK>(v, sh);     // thread 0 ends with the minimum of the workgroup
    if (threadIdx.x == 0) sh[0] = v;
    __syncthreads();
    v = sh[0];
    __syncthreads();
    return v;
}

// ---- 1. tile summaries --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DB_BLOCK) void k_db_tiles(const uint8_t *__restrict__ in, int64_t n, TileArrays ta)
{
    __shared__ int64_t sh[DB_BLOCK];
    const int64_t tile = blockIdx.x;
    const int64_t p0 = tile * DB_TILE + (int64_t)threadIdx.x * DB_PER;
    uint8_t c[DB_PER];
    load16(in, p0, n, c);
    int sum = 0;
    int64_t last_nd = -1, first_nd = DB_NONE, last_sep = -1, first_sep = DB_NONE;
#pragma unroll
    for (int k = 0; k < DB_PER; ++k) {
        const int64_t p = p0 + k;
        if (p >= n) break;
        sum += delta_of(c[k]);
        if (c[k] != C_DOT) {
            last_nd = (p << 3) | (c[k] & 7);
            if (first_nd == DB_NONE) first_nd = (p << 3) | (c[k] & 7);
        }
        if (c[k] == C_SEP) {
            last_sep = p;
            if (first_sep == DB_NONE) first_sep = p;
        }
    }
    const int64_t s = scan_sum<DB_BLOCK>(sum, sh);
    const int64_t lnd = scan_max<DB_BLOCK>(last_nd, sh);
    const int64_t lsp = scan_max<DB_BLOCK>(last_sep, sh);
    const int64_t fnd = scan_min_suffix<DB_BLOCK>(first_nd, sh);
    const int64_t fsp = scan_min_suffix<DB_BLOCK>(first_sep, sh);
    if (threadIdx.x == DB_BLOCK - 1) {
        ta.sum[tile] = (int32_t)s;
        ta.last_nd[tile] = lnd;
        ta.last_sep[tile] = lsp;
    }
    if (threadIdx.x == 0) {
        ta.first_nd[tile] = fnd;
        ta.first_sep[tile] = fsp;
    }
}

// ---- 2. one workgroup scans the tile summaries ----------------------------------------------------------------------
__global__ __launch_bounds__(DB_SCAN_BLOCK) void k_db_scan(int64_t nt, int64_t n, TileArrays ta, Flags *flags)
{
    __shared__ int64_t sh[DB_SCAN_BLOCK];
    const int64_t chunk = (nt + DB_SCAN_BLOCK - 1) / DB_SCAN_BLOCK;
    const int64_t lo = min(nt, (int64_t)threadIdx.x * chunk), hi = min(nt, lo + chunk);
    int64_t sum = 0, lnd = -1, lsp = -1, fnd = DB_NONE;
    for (int64_t t = lo; t < hi; ++t) {
        sum += ta.sum[t];
        lnd = max(lnd, ta.last_nd[t]);
        lsp = max(lsp, ta.last_sep[t]);
        fnd = min(fnd, ta.first_nd[t]);
    }
    // exclusive forms: what lies before this thread's chunk (after it, for the suffix minimum)
    const int64_t ex_sum = scan_sum<DB_SCAN_BLOCK>(sum, sh) - sum;
    int64_t ex_lnd = scan_max<DB_SCAN_BLOCK>(lnd, sh);
    int64_t ex_lsp = scan_max<DB_SCAN_BLOCK>(lsp, sh);
    int64_t ex_fnd = scan_min_suffix<DB_SCAN_BLOCK>(fnd, sh);
    // shift by one thread: inclusive value of the neighbour
    sh[threadIdx.x] = ex_lnd;
    __syncthreads();
    ex_lnd = threadIdx.x ? sh[threadIdx.x - 1] : -1;
    __syncthreads();
    sh[threadIdx.x] = ex_lsp;
    __syncthreads();
    ex_lsp = threadIdx.x ? sh[threadIdx.x - 1] : -1;
    const int64_t total_lsp = sh[DB_SCAN_BLOCK - 1];
    __syncthreads();
    sh[threadIdx.x] = ex_fnd;
    __syncthreads();
    ex_fnd = threadIdx.x + 1 < DB_SCAN_BLOCK ? sh[threadIdx.x + 1] : DB_NONE;
    __syncthreads();

    int64_t run_sum = ex_sum, run_lnd = ex_lnd, run_lsp = ex_lsp;
    int64_t bad_long = DB_NONE;
    for (int64_t t = lo; t < hi; ++t) {
        ta.pre[t] = run_sum;
        ta.prev_nd[t] = run_lnd;
        const int64_t fs = ta.first_sep[t];
        if (fs != DB_NONE && fs - run_lsp - 1 >= DB_MAX_RECORD) bad_long = min(bad_long, fs);
        run_sum += ta.sum[t];
        run_lnd = max(run_lnd, ta.last_nd[t]);
        run_lsp = max(run_lsp, ta.last_sep[t]);
    }
    int64_t run_fnd = ex_fnd;
    for (int64_t t = hi - 1; t >= lo; --t) {
        ta.next_nd[t] = run_fnd;
        run_fnd = min(run_fnd, ta.first_nd[t]);
    }
    if (threadIdx.x == 0 && n - 1 - total_lsp >= DB_MAX_RECORD) bad_long = min(bad_long, n - 1);   // no separator at the end
    if (bad_long != DB_NONE) atomicMin(reinterpret_cast<unsigned long long *>(&flags->first_long), (unsigned long long)bad_long);
}

// ---- 3. depth, validity, min-tree levels 1 and 2 --------------------------------------------------------------------
__global__ __launch_bounds__(DB_BLOCK) void k_db_depth(const uint8_t *__restrict__ in, int64_t n, TileArrays ta, Tree tr,
                                                       Flags *flags)
{
    __shared__ int64_t sh[DB_BLOCK];
    const int64_t tile = blockIdx.x;
    const int64_t p0 = tile * DB_TILE + (int64_t)threadIdx.x * DB_PER;
    uint8_t c[DB_PER];
    load16(in, p0, n, c);
    int sum = 0;
#pragma unroll
    for (int k = 0; k < DB_PER; ++k) sum += (p0 + k < n) ? delta_of(c[k]) : 0;
    int64_t d = ta.pre[tile] + scan_sum<DB_BLOCK>(sum, sh) - sum;     // depth before this thread's first position
    int32_t *depth = tr.base;                                         // level 0
    int64_t bad = DB_NONE;
    int32_t mn = INT32_MAX;
#pragma unroll
    for (int k = 0; k < DB_PER; ++k) {
        const int64_t p = p0 + k;
        if (p >= n) break;
        const uint8_t x = c[k];
        d += delta_of(x);
        const bool ok = (x == C_DOT || x == C_OPEN || x == C_CLOSE || x == C_SEP) && d >= 0 && (x != C_SEP || d == 0) &&
                        (p != n - 1 || x == C_SEP);
        if (!ok && bad == DB_NONE) bad = p;
        const int32_t d32 = (int32_t)min(d, (int64_t)INT32_MAX);
        depth[p] = d32;
        mn = min(mn, d32);
    }
    // level 1: 64 positions = 4 threads (lanes 4q .. 4q + 3 of the wave)
    mn = min(mn, __shfl_xor(mn, 1));
    mn = min(mn, __shfl_xor(mn, 2));
    const int64_t q1 = p0 / 64;
    if ((threadIdx.x & 3) == 0 && q1 < tr.cnt[1]) tr.base[tr.off[1] + q1] = mn;
    // level 2: the tile
    const int64_t tmn = block_min(mn, sh);
    if (threadIdx.x == 0 && tile < tr.cnt[2]) tr.base[tr.off[2] + tile] = (int32_t)tmn;
    const int64_t first = block_min(bad, sh);
    if (threadIdx.x == 0 && first != DB_NONE)
        atomicMin(reinterpret_cast<unsigned long long *>(&flags->first_bad), (unsigned long long)first);
}

__global__ __launch_bounds__(DB_BLOCK) void k_db_level(int32_t *__restrict__ base, int64_t off_in, int64_t n_in,
                                                       int64_t off_out, int64_t n_out)
{
    const int64_t q = (int64_t)blockIdx.x * DB_BLOCK + threadIdx.x;
    if (q >= n_out) return;
    const int64_t lo = q * 64, hi = min(lo + 64, n_in);
    int32_t mn = INT32_MAX;
    for (int64_t x = lo; x < hi; ++x) mn = min(mn, base[off_in + x]);
    base[off_out + q] = mn;
}

// ---- 4. partners ----------------------------------------------------------------------------------------------------
// first index > q at level l whose minimum is below target, descended to level 0 (a position), or -1: scan the rest of q's
// group of 64 at each level going up, then descend into the first entry below target.  Bounded by cnt[] at every level.
__device__ int64_t next_smaller(const int32_t *__restrict__ base, const int64_t *s_off, const int64_t *s_cnt, int nl,
                                int l, int64_t q, int32_t target)
{
    for (;;) {
        const int64_t len = s_cnt[l];
        const int64_t end = (l == nl - 1) ? len : min((q / 64 + 1) * 64, len);
        const int32_t *v = base + s_off[l];
        int64_t x = q + 1;
        while (x < end && v[x] >= target) ++x;
        if (x < end) {
            q = x;
            break;
        }
        if (l >= nl - 1) return -1;
        q /= 64;
        ++l;
    }
    while (l > 0) {
        const int64_t lo = q * 64, hi = min(lo + 64, s_cnt[l - 1]);
        const int32_t *v = base + s_off[l - 1];
        int64_t x = lo;
        while (x < hi && v[x] >= target) ++x;
        if (x >= hi) return -1;                   // inconsistent tree: cannot happen after k_db_depth / k_db_level
        q = x;
        --l;
    }
    return q;
}

// One workgroup per tile: the tile's depths and its 64 group minima in LDS answer every pair that closes inside the tile
// (most stems close within a few hundred positions); the rest climb the global tree from the tile's level.
__global__ __launch_bounds__(DB_BLOCK) void k_db_pairs(const uint8_t *__restrict__ in, int64_t n, Tree tr,
                                                       int32_t *__restrict__ part)
{
    __shared__ int64_t s_off[DB_MAXL], s_cnt[DB_MAXL];
    __shared__ int32_t s_d[DB_TILE];
    __shared__ int32_t s_m1[64];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < DB_MAXL; ++l) {
            s_off[l] = tr.off[l];
            s_cnt[l] = tr.cnt[l];
        }
    }
    const int64_t tile = blockIdx.x;
    const int64_t base = tile * DB_TILE;
    const int len = (int)min((int64_t)DB_TILE, n - base);
    for (int k = threadIdx.x; k < len; k += DB_BLOCK) s_d[k] = tr.base[base + k];
    if (threadIdx.x < 64) {
        const int64_t g = tile * 64 + threadIdx.x;
        s_m1[threadIdx.x] = (threadIdx.x * 64 < len && g < tr.cnt[1]) ? tr.base[tr.off[1] + g] : INT32_MAX;
    }
    __syncthreads();
    const int ng = (len + 63) >> 6;
    for (int r = 0; r < DB_PER; ++r) {            // strided: the lanes of a wave search side by side
        const int li = r * DB_BLOCK + threadIdx.x;
        if (li >= len || in[base + li] != C_OPEN) continue;
        const int32_t target = s_d[li];           // depth after the '(' = d + 1; its partner is the first depth d after it
        int64_t j = -1;
        int x = li + 1;
        const int gend = min((li | 63) + 1, len);
        while (x < gend && s_d[x] >= target) ++x;
        if (x < gend) {
            j = base + x;
        } else {
            int g = (li >> 6) + 1;
            while (g < ng && s_m1[g] >= target) ++g;
            if (g < ng) {
                x = g * 64;
                const int e = min(x + 64, len);
                while (x < e && s_d[x] >= target) ++x;
                if (x < e) j = base + x;
            } else if (tr.nl > 2) {
                j = next_smaller(tr.base, s_off, s_cnt, tr.nl, 2, tile, target);
            }
        }
        if (j < 0 || j >= n || j - (base + li) >= DB_MAX_RECORD || in[j] != C_CLOSE) continue;   // not on a valid stream
        part[base + li] = (int32_t)(j - (base + li));
        part[j] = (int32_t)((base + li) - j);
    }
}

// ---- 5. labels ------------------------------------------------------------------------------------------------------
__device__ inline void mark_run(const uint8_t *__restrict__ in, uint8_t *__restrict__ marks, int64_t n, int64_t x)
{
    if (x >= 0 && x < n && in[x] == C_DOT) marks[x] = 1;
}

// PASS 0: rule 3's marks.  PASS 1: the labels, N resolved by the marks, written through `map` (8 bytes: code of E, H, T,
// B, L, R, M, separator), and the histogram of the written codes.
template <int PASS>
__global__ __launch_bounds__(DB_BLOCK) void k_db_label(const uint8_t *__restrict__ in, int64_t n, TileArrays ta, Tree tr,
                                                       const int32_t *__restrict__ part, uint8_t *__restrict__ marks,
                                                       uint8_t *__restrict__ out, uint64_t map, Flags *flags)
{
    __shared__ int64_t sh[DB_BLOCK];
    __shared__ int s_count[8];
    const int64_t tile = blockIdx.x;
    const int64_t p0 = tile * DB_TILE + (int64_t)threadIdx.x * DB_PER;
    uint8_t c[DB_PER];
    load16(in, p0, n, c);
    int64_t last = -1, first = DB_NONE;           // this thread's last / first non-dot (pos << 3 | code)
#pragma unroll
    for (int k = 0; k < DB_PER; ++k) {
        const int64_t p = p0 + k;
        if (p < n && c[k] != C_DOT) {
            last = (p << 3) | (c[k] & 7);
            if (first == DB_NONE) first = last;
        }
    }
    int64_t left = scan_max<DB_BLOCK>(last, sh);
    int64_t right = scan_min_suffix<DB_BLOCK>(first, sh);
    // exclusive: the neighbour's inclusive value, seeded with what lies outside the tile
    sh[threadIdx.x] = left;
    __syncthreads();
    left = threadIdx.x ? sh[threadIdx.x - 1] : -1;
    __syncthreads();
    sh[threadIdx.x] = right;
    __syncthreads();
    right = threadIdx.x + 1 < DB_BLOCK ? sh[threadIdx.x + 1] : DB_NONE;
    if (PASS == 1 && threadIdx.x < 8) s_count[threadIdx.x] = 0;
    __syncthreads();
    left = max(left, ta.prev_nd[tile]);
    right = min(right, ta.next_nd[tile]);

    // nearest non-dot right of each of this thread's positions (walk backwards)
    int64_t rnd[DB_PER];
#pragma unroll
    for (int k = DB_PER - 1; k >= 0; --k) {
        rnd[k] = right;
        const int64_t p = p0 + k;
        if (p < n && c[k] != C_DOT) right = (p << 3) | (c[k] & 7);
    }
    uint64_t cnt = 0;                             // 7 bit-fields of 5 bits: this thread's count per output letter
#pragma unroll
    for (int k = 0; k < DB_PER; ++k) {
        const int64_t p = p0 + k;
        if (p >= n) break;
        const uint8_t x = c[k];
        int lab;
        if (x == C_OPEN) {
            lab = L_L;
        } else if (x == C_CLOSE) {
            lab = L_R;
            // rule 3 with s[j + 1] == '(' (step-2 label L): m = j + 1
            const int64_t nx = rnd[k];
            if (PASS == 0 && nx != DB_NONE && (nx >> 3) == p + 1 && (nx & 7) == C_OPEN) {
                mark_run(in, marks, n, p + part[p] - 1);
                mark_run(in, marks, n, p + 1 + part[p + 1] + 1);
            }
        } else if (x == C_DOT) {
            const int64_t kk = left < 0 ? -1 : (left >> 3), mm = rnd[k] == DB_NONE ? n : (rnd[k] >> 3);
            const int kc = left < 0 ? C_SEP : (int)(left & 7), mc = rnd[k] == DB_NONE ? C_SEP : (int)(rnd[k] & 7);
            if (kc == C_SEP || mc == C_SEP || mm >= n) {
                lab = L_E;
            } else if (kc == C_OPEN && mc == C_CLOSE) {
                lab = L_H;
            } else if (kc == C_CLOSE && mc == C_OPEN) {
                lab = tr.base[p] > 0 ? L_M : L_E;
                // rule 3 with a dot run at j + 1 (step-2 label M): j = k, m = the run's right bracket; once per run
                if (PASS == 0 && lab == L_M && kk == p - 1) {
                    mark_run(in, marks, n, kk + part[kk] - 1);
                    mark_run(in, marks, n, mm + part[mm] + 1);
                }
            } else if (kc == mc && (kc == C_OPEN || kc == C_CLOSE)) {
                lab = (mm + part[mm] + 1 == kk + part[kk]) ? L_B : L_N;
                if (PASS == 1 && lab == L_N) lab = (marks[kk + 1] | marks[mm - 1]) ? L_M : L_T;
            } else {
                lab = L_E;                        // not reached on a valid stream
            }
        } else {
            lab = -1;                             // separator
        }
        if (PASS == 1) {
            if (lab < 0) {
                out[p] = (uint8_t)(map >> 56);
            } else {
                const int code = (int)((map >> (8 * lab)) & 0xff);
                out[p] = (uint8_t)code;
                cnt += (uint64_t)1 << (5 * code);
            }
        }
        if (x != C_DOT) left = (p << 3) | (x & 7);
    }
    if (PASS == 1) {
#pragma unroll
        for (int l = 0; l < 7; ++l) {
            const int v = (int)((cnt >> (5 * l)) & 31);
            if (v) atomicAdd(&s_count[l], v);
        }
        __syncthreads();
        if (threadIdx.x < 7 && s_count[threadIdx.x])
            atomicAdd(reinterpret_cast<unsigned long long *>(&flags->counts[threadIdx.x]), (unsigned long long)s_count[threadIdx.x]);
    }
}

struct Scratch {
    TileArrays ta;
    Tree tr;
    int32_t *part;
    uint8_t *marks;
    Flags *flags;
};

int prepare(pfmscan_ctx *ctx, int64_t n, Scratch &s)
{
    const int64_t nt = (n + DB_TILE - 1) / DB_TILE;
    // min-tree layout: level l at off[l], 64-aligned
    Tree tr{};
    int64_t at = 0, cnt = n;
    int nl = 0;
    for (;;) {
        tr.off[nl] = at;
        tr.cnt[nl] = cnt;
        at += (cnt + 63) / 64 * 64;
        ++nl;
        if (nl >= 3 && cnt <= 64) break;          // levels 1 and 2 always exist (k_db_depth writes them)
        if (nl == DB_MAXL) return fail(ctx, PFMSCAN_E_BADSHAPE, "dot-bracket stream too long");
        cnt = (cnt + 63) / 64;
    }
    // the search needs no level above the first one that fits in one group of 64
    tr.nl = 1;
    while (tr.cnt[tr.nl - 1] > 64) ++tr.nl;
    for (int l = nl; l < DB_MAXL; ++l) tr.off[l] = tr.cnt[l] = 0;
    int rc;
    if ((rc = ensure(ctx, ctx->db_tree, (size_t)at * sizeof(int32_t)))) return rc;
    if ((rc = ensure(ctx, ctx->db_part, (size_t)n * sizeof(int32_t)))) return rc;
    if ((rc = ensure(ctx, ctx->db_marks, (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->db_tiles, (size_t)nt * (sizeof(int32_t) + 7 * sizeof(int64_t)) + 64))) return rc;
    if ((rc = ensure(ctx, ctx->db_flags, sizeof(Flags)))) return rc;
    tr.base = static_cast<int32_t *>(ctx->db_tree.p);
    int64_t *t64 = static_cast<int64_t *>(ctx->db_tiles.p);
    s.ta.last_nd = t64;
    s.ta.first_nd = t64 + nt;
    s.ta.last_sep = t64 + 2 * nt;
    s.ta.first_sep = t64 + 3 * nt;
    s.ta.pre = t64 + 4 * nt;
    s.ta.prev_nd = t64 + 5 * nt;
    s.ta.next_nd = t64 + 6 * nt;
    s.ta.sum = reinterpret_cast<int32_t *>(t64 + 7 * nt);
    s.tr = tr;
    s.part = static_cast<int32_t *>(ctx->db_part.p);
    s.marks = static_cast<uint8_t *>(ctx->db_marks.p);
    s.flags = static_cast<Flags *>(ctx->db_flags.p);
    return PFMSCAN_OK;
}

}  // namespace

namespace pfmscan {

// d_in -> d_out on `st`.  Synchronises `st` once, after the validity pass.  *first_bad = -1, or the first invalid
// position (PFMSCAN_E_BADARG; PFMSCAN_E_BADSHAPE for a record of 2^31 positions or more).  d_counts: device int64 [7] or
// NULL; host_counts: host int64 [7] or NULL (then `st` is synchronised again).
int dotbracket_annotate(pfmscan_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, int64_t n, const uint8_t *map,
                        int64_t *d_counts, int64_t *host_counts, int64_t *first_bad, hipStream_t st)
{
    if (first_bad) *first_bad = -1;
    if (!map) return fail(ctx, PFMSCAN_E_BADARG, "dot-bracket annotation: NULL map");
    uint64_t mapw = (uint64_t)PFMSCAN_SEP << 56;
    for (int l = 0; l < 7; ++l) {
        if (map[l] >= PFMSCAN_SEP) return fail(ctx, PFMSCAN_E_BADARG, "dot-bracket annotation: map entries must be 0..6");
        mapw |= (uint64_t)map[l] << (8 * l);
    }
    if (n < 0) return fail(ctx, PFMSCAN_E_BADARG, "negative n_pos");
    if (n > 0 && (!d_in || !d_out)) return fail(ctx, PFMSCAN_E_BADARG, "dot-bracket annotation: NULL stream");
    if (n > 0 && d_in == d_out) return fail(ctx, PFMSCAN_E_BADARG, "dot-bracket annotation: d_in and d_out must not alias");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (d_counts) HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, 7 * sizeof(int64_t), st));
    if (n == 0) {
        if (host_counts)
            for (int l = 0; l < 7; ++l) host_counts[l] = 0;
        return PFMSCAN_OK;
    }
    Scratch s;
    int rc = prepare(ctx, n, s);
    if (rc) return rc;
    const int64_t nt = (n + DB_TILE - 1) / DB_TILE;
    int64_t *d_hist = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(s.flags) + offsetof(Flags, counts));
    HIP_TRY(ctx, hipMemsetAsync(s.flags, 0x7f, offsetof(Flags, counts), st));      // 0x7f7f..: "no bad position"
    HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, 8 * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_db_tiles, dim3((unsigned)nt), dim3(DB_BLOCK), 0, st, d_in, n, s.ta);
    hipLaunchKernelGGL(k_db_scan, dim3(1), dim3(DB_SCAN_BLOCK), 0, st, nt, n, s.ta, s.flags);
    hipLaunchKernelGGL(k_db_depth, dim3((unsigned)nt), dim3(DB_BLOCK), 0, st, d_in, n, s.ta, s.tr, s.flags);
    for (int l = 3; l < DB_MAXL && s.tr.cnt[l] > 0; ++l)
        hipLaunchKernelGGL(k_db_level, dim3((unsigned)((s.tr.cnt[l] + DB_BLOCK - 1) / DB_BLOCK)), dim3(DB_BLOCK), 0, st,
                           s.tr.base, s.tr.off[l - 1], s.tr.cnt[l - 1], s.tr.off[l], s.tr.cnt[l]);
    HIP_TRY(ctx, hipGetLastError());
    int64_t verdict[2];
    HIP_TRY(ctx, hipMemcpyAsync(verdict, s.flags, sizeof(verdict), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (verdict[0] < n) {
        if (first_bad) *first_bad = verdict[0];
        return fail(ctx, PFMSCAN_E_BADARG, "invalid dot-bracket record at stream position " + std::to_string(verdict[0]) +
                                               ": a character outside '().', an unbalanced bracket or a missing separator");
    }
    if (verdict[1] < n) {
        if (first_bad) *first_bad = verdict[1];
        return fail(ctx, PFMSCAN_E_BADSHAPE, "dot-bracket record of 2^31 positions or more ending at stream position " +
                                                 std::to_string(verdict[1]));
    }
    hipLaunchKernelGGL(k_db_pairs, dim3((unsigned)nt), dim3(DB_BLOCK), 0, st, d_in, n, s.tr, s.part);
    HIP_TRY(ctx, hipMemsetAsync(s.marks, 0, (size_t)n, st));
    hipLaunchKernelGGL(k_db_label<0>, dim3((unsigned)nt), dim3(DB_BLOCK), 0, st, d_in, n, s.ta, s.tr, s.part, s.marks,
                       d_out, mapw, s.flags);
    hipLaunchKernelGGL(k_db_label<1>, dim3((unsigned)nt), dim3(DB_BLOCK), 0, st, d_in, n, s.ta, s.tr, s.part, s.marks,
                       d_out, mapw, s.flags);
    HIP_TRY(ctx, hipGetLastError());
    if (d_counts) HIP_TRY(ctx, hipMemcpyAsync(d_counts, d_hist, 7 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (host_counts) {
        HIP_TRY(ctx, hipMemcpyAsync(host_counts, d_hist, 7 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return PFMSCAN_OK;
}

}  // namespace pfmscan

extern "C" {

int pfmscan_dotbracket_annotate_dev(pfmscan_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, int64_t n_pos,
                                    const uint8_t *map, int64_t *d_counts, int64_t *first_bad, void *stream)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    return dotbracket_annotate(ctx, d_in, d_out, n_pos, map, d_counts, nullptr, first_bad,
                               stream ? (hipStream_t)stream : ctx->stream);
}

int pfmscan_dotbracket_stage(pfmscan_ctx *ctx, const uint8_t *codes, int64_t n_pos, int which, const uint8_t *map,
                             int64_t *counts, int64_t *first_bad)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    if (n_pos < 0) return fail(ctx, PFMSCAN_E_BADARG, "negative n_pos");
    if (which != 0 && which != 1) return fail(ctx, PFMSCAN_E_BADARG, "which must be 0 (the codes slot) or 1 (codes2)");
    if (n_pos > 0 && !codes) return fail(ctx, PFMSCAN_E_BADARG, "codes is NULL");
    if (which == 1) {
        if (ctx->staged_n < 0 || !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, "no code stream staged (call pfmscan_stage first)");
        if (n_pos != ctx->staged_n) return fail(ctx, PFMSCAN_E_BADARG, "the second code stream must have the staged stream's length");
        ctx->staged_codes2 = false;
    } else {
        ctx->staged_n = -1;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf &dst = which == 0 ? ctx->codes : ctx->codes2;
    int rc;
    if (n_pos > 0) {
        if ((rc = ensure(ctx, ctx->db_in, (size_t)n_pos))) return rc;
        if ((rc = ensure(ctx, dst, (size_t)n_pos))) return rc;
        if ((rc = upload(ctx, ctx->db_in.p, codes, (size_t)n_pos, ctx->stream))) return rc;
    }
    int64_t tmp[7];
    rc = dotbracket_annotate(ctx, static_cast<const uint8_t *>(ctx->db_in.p), static_cast<uint8_t *>(dst.p), n_pos, map,
                             nullptr, counts ? counts : tmp, first_bad, ctx->stream);
    if (rc) return rc;
    if (which == 0) {
        ctx->staged_n = n_pos;
        ++ctx->stage_serial;
        ctx->staged_dtype = PFMSCAN_PROFILE_NONE;
        ctx->staged_codes = true;
        ctx->staged_profile = false;
        ctx->staged_codes2 = false;
    } else {
        ctx->staged_codes2 = true;
    }
    return PFMSCAN_OK;
}

int pfmscan_dotbracket_annotate_host(pfmscan_ctx *ctx, const uint8_t *in, uint8_t *out, int64_t n_pos, const uint8_t *map,
                                     int64_t *counts, int64_t *first_bad)
{
    if (first_bad) *first_bad = -1;
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx");
    if (n_pos < 0) return fail(ctx, PFMSCAN_E_BADARG, "negative n_pos");
    if (n_pos > 0 && (!in || !out)) return fail(ctx, PFMSCAN_E_BADARG, "NULL in / out");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if (n_pos > 0) {
        if ((rc = ensure(ctx, ctx->db_in, (size_t)n_pos))) return rc;
        if ((rc = ensure(ctx, ctx->db_out, (size_t)n_pos))) return rc;
        if ((rc = upload(ctx, ctx->db_in.p, in, (size_t)n_pos, ctx->stream))) return rc;
    }
    int64_t tmp[7];
    rc = dotbracket_annotate(ctx, static_cast<const uint8_t *>(ctx->db_in.p), static_cast<uint8_t *>(ctx->db_out.p), n_pos,
                             map, nullptr, counts ? counts : tmp, first_bad, ctx->stream);
    if (rc) return rc;
    if (n_pos > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(out, ctx->db_out.p, (size_t)n_pos, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PFMSCAN_OK;
}

}  // extern "C"
