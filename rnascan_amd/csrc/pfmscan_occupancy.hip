// pfmscan_occupancy.hip -- occupancy: the summed likelihood ratio of every record under every motif.
//
// R [m][8] holds the motif's odds ratios p / b (pssm.odds): +0.0, positive, +inf or NaN, never negative.  The term of window s
// is t = R[0][c_0], then t = t * R[k][c_k] for k ascending, every product rounded to double (c_k = codes[s + k] & 7); a window
// that holds a code >= n_letters has no term.  The occupancy of a record is the sum of its n_win = max(L - m + 1, 0) terms
// (skipped windows as +0.0) in a left-aligned tree of fan-in PFMSCAN_OCC_FANIN = 32 anchored at the record's first window:
// element j of the next level is a[32 j], + a[32 j + 1], ... over the children that exist, sequential and each rounded.  No
// transcendental, no atomics, no tolerance: tests/occupancy_rules.py restates it in numpy and the bits are compared.
//
//   k_occ_blocks<QN, PAIR>   level 0.  A lane owns one (record, block of 32 consecutive windows) and walks the windows
//                      serially for QN = 8, 4, 2 or 1 motifs at a time: 0.0 + t_0 + t_1 ... is the definition's sum (x + +0.0
//                      == x for every value a term can take, so a skipped window adds nothing).  The block's 32 + m - 1 codes
//                      sit in a lane-private strip of LDS an odd number of dwords wide (aligned dwords as loaded, foreign
//                      codes zeroed and kept as a 128-bit mask in registers: no register array is indexed at run time); the
//                      ratio tables of a chunk of motifs sit in LDS transposed [row][letter][motif], so one letter serves
//                      QN adjacent motifs with 16-byte reads.  PAIR: two code streams, both codes of a
//                      position packed into one byte of the strip and the letter chain continued over the structure
//                      letters; described above the kernel, with the rule for the pairs of an LDS chunk.
//   k_occ_level1       level 1: a thread adds the <= 32 block sums of one (group of 32 blocks, motif), in order.
//   k_occ_finish       levels 2 and up: a thread per (record, motif) folds the record's level-1 sums in place, in order, and
//                      writes the cell.  One writer per cell.
// The block sums go through scratch that is bounded (OCC_SCRATCH_DOUBLES) by running the records, and if one record alone is
// too long the motifs, in passes: the plan is occ_plan (pfmscan_occ_plan.hpp), here over motifs.  What the expected counts
// (pfmscan_expect.hip, pfmscan_expect_profile.hip) share -- the arguments of a pass and the frame that fills them, the bisection,
// levels 1 and up, whose n_q columns are then the cells of motifs, and the pieces of the entry points -- is declared in
// pfmscan_occ.hpp and defined here.
//
// Averaged-structure profiles (include/pfmscan.h "occupancy on averaged-structure profiles"): the term of a
// window is the product over k of the marginal d(s + k, k) = sum_c r[s + k][c] * S[k][c] (7 rounded products, 6 rounded
// additions, ascending c), in joint mode continued from the letter chain above.  Only level 0 differs:
//   k_occ_profile_blocks<T, SEQ, QN>   a workgroup owns a run of 8 consecutive blocks of one record (256 windows, a lane per
//                      window).  The run's 256 + m - 1 rows are fetched as the aligned 16-byte vectors that cover them and
//                      parked in LDS as doubles; for every k a lane holds its row's 7 doubles in registers and advances the
//                      product chains of QN motifs, whose table rows are workgroup-uniform (scalar loads).  The QN x 256
//                      terms go to LDS (a block's 32 terms one double apart from the next block's: the serial readers fall
//                      on different banks) and one lane per (block, motif) adds the 32 in order.  A workgroup walks up to
//                      OCCP_CHUNK motifs over the rows it staged; gridDim.y covers the rest.
//   k_occ_run_records  before it, per pass: a thread per record writes the record of each of its runs (a third prefix table,
//                      ceil(blocks / 8) per record, numbers the runs), so that a workgroup does not bisect that table.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_occ.hpp"

#pragma clang fp contract(off)   // the product chain and the sums are rounded one operation at a time: never an FMA

namespace pfmscan {

// table cells of one chunk of motifs, padding included (occ_chunk).  Measured: 256 motifs of w = 12 at C2 size take 70.4 ms
// with 2048, 74.8 with 4096, 72.1 with 1024 (profiles/occupancy/NOTES.md)
constexpr int OCC_LDS_DOUBLES = 2048;
static_assert(OCC_LDS_DOUBLES >= PFMSCAN_MAX_M * PFMSCAN_NSTRUCT, "one motif of the widest kind fits");
constexpr int OCC_CODE_DWORDS = 25;                   // aligned dwords that cover 3 + 32 + PFMSCAN_MAX_M - 1 bytes
static_assert(OCC_CODE_DWORDS * 4 >= 3 + OCC_FANIN + PFMSCAN_MAX_M - 1, "strip");

// dwords of a lane's strip of codes: the aligned dwords that cover 3 + 32 + m - 1 bytes, made odd so that the byte reads of
// the 32 lanes of a group fall on 32 banks
__host__ __device__ inline int occ_strip(int m) { return ((3 + OCC_FANIN + m - 1 + 3) / 4) | 1; }

__host__ __device__ inline int occ_ls(int nq, int qn)
{
    int ls = (nq + qn - 1) / qn * qn;
    return ls % 16 == 0 ? ls + 2 : ls;                // the letters of a row must not all start on one bank
}

// QN adjacent motifs' cells of one (row, letter): 16-byte reads (ls is even and q a multiple of QN)
template <int QN>
__device__ __forceinline__ void occ_cells(const double *p, double (&v)[QN])
{
    if constexpr (QN == 1) {
        v[0] = p[0];
    } else {
#pragma unroll
        for (int i = 0; i < QN; i += 2) {
            const double2 x = *reinterpret_cast<const double2 *>(p + i);
            v[i] = x.x;
            v[i + 1] = x.y;
        }
    }
}

// ---- level 0 on letter strings, and on two code streams (include/pfmscan.h "occupancy and expected counts of
// two code streams") --------------------------------------------------------------------------------------------------------
// PAIR: the term of a window is the letter chain over codes (4 RNA letters) continued by the letter chain over codes2 (7
// structure letters), 2 m - 1 rounded products, letters first.  Both codes of a position share ONE byte of the lane's strip --
// bits 0..2 the RNA code, bits 3..5 the structure code, a position that is foreign in either stream zeroed and remembered in
// the 128-bit mask -- so the byte traffic of the strip and its size are those of one stream (a second strip would double the
// reads of an LDS-bound kernel and pass 64 KB of dynamic LDS at m = 64).  The tables of a chunk of pairs sit in LDS as
// [row][letter][pair] with OCC_PAIR_LETTERS = 4 + 7 letters per row: 0..3 the row of R, 4..10 the row of S.  The products
// R[k][a] * S[k][b] are never made: that would be another rounding.
// Chunk rule (occ_chunk, with 11 letters for pairs): the most motifs c <= n_q with m * letters * occ_ls(c, occ_qn(c)) <=
// OCC_LDS_DOUBLES, at least 1; occ_qn(c) = 8, 4, 2, 1 for c >= 8, 4, 2, 1 and occ_ls(c, qn) = c rounded up to a multiple of qn,
// plus 2 when that is a multiple of 16.
constexpr int OCC_PAIR_LETTERS = 4 + PFMSCAN_NSTRUCT;
static_assert(OCC_LDS_DOUBLES >= PFMSCAN_MAX_M * OCC_PAIR_LETTERS, "one pair of the widest kind fits");

// the aligned dword at p of a stream of n_pos codes (the base pointer is 16-byte aligned); the stream's last one may be cut short
__device__ __forceinline__ uint32_t occ_dword(const uint8_t *__restrict__ codes, int64_t p, int64_t n_pos)
{
    if (p + 4 <= n_pos) return *reinterpret_cast<const uint32_t *>(codes + p);
    uint32_t dw = 0;
    for (int j = 0; j < 4; ++j)
        if (p + j < n_pos) dw |= (uint32_t)codes[p + j] << (8 * j);
    return dw;
}

template <int QN, bool PAIR>
__global__ __launch_bounds__(BLOCK) void k_occ_blocks(const OccArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char occ_lds[];
    const int m = a.m, nl = PAIR ? OCC_PAIR_LETTERS : a.n_letters;
    const int cs = occ_strip(m);                                   // dwords per lane strip
    uint32_t *cw = reinterpret_cast<uint32_t *>(occ_lds);          // [BLOCK][cs]
    double *lt = reinterpret_cast<double *>(occ_lds + (size_t)BLOCK * cs * 4);   // [m][nl][ls]; BLOCK * 4 is a multiple of 16
    const int qc = (int)blockIdx.y * a.chunk;                      // first motif of the chunk, within the pass
    const int nq = min(a.chunk, a.n_q - qc);
    const int ls = occ_ls(a.chunk, QN);
    for (int i = threadIdx.x; i < m * nl * ls; i += BLOCK) {
        const int r = i / ls, q = i - r * ls;                      // r = row * nl + letter
        const int row = r / nl, c = r - row * nl;
        const bool second = PAIR && c >= 4;                        // a letter of the structure table
        const double *src = second ? a.tables2 : a.tables;
        lt[i] = q < nq ? src[((int64_t)(a.q_first + qc + q) * m + row) * 8 + (second ? c - 4 : c)] : 0.0;
    }
    // this lane's block: its codes as aligned dwords into the lane's strip, foreign codes zeroed and remembered
    const int64_t gb = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t valid = 0;                                            // bit w: window w of the block has a term
    int sh = 0;
    if (gb < a.n_blk) {
        const int64_t b = a.blk_base + gb;
        const int64_t r = occ_record(a.blk_start, a.r0, a.r1, b);
        const int64_t w0 = (b - a.blk_start[r]) * OCC_FANIN;
        const int64_t left = a.rec_len[r] - m + 1 - w0;            // >= 1: the block exists
        const int nw = (int)min((int64_t)OCC_FANIN, left);
        const int need = nw + m - 1;                               // codes of the block, all inside the record
        const int64_t s0 = a.rec_off[r] + w0;
        sh = (int)(s0 & 3);
        const int64_t base = s0 - sh;
        unsigned long long f0 = 0, f1 = 0;                         // bit i: code i of the block is foreign (in either stream) or not the block's
        uint32_t *mine = cw + threadIdx.x * cs;
#pragma unroll
        for (int i = 0; i < OCC_CODE_DWORDS; ++i) {
            const int64_t p = base + 4 * i;
            uint32_t d1 = 0, d2 = 0;
            if (4 * i - sh < need) {
                d1 = occ_dword(a.codes, p, a.n_pos);
                if constexpr (PAIR) d2 = occ_dword(a.codes2, p, a.n_pos);
            }
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = 4 * i + j - sh;                    // -3 .. 99
                const uint32_t c1 = (d1 >> (8 * j)) & 7u, c2 = (d2 >> (8 * j)) & 7u;
                const bool bad = idx >= need || (PAIR ? c1 >= 4u || c2 >= (uint32_t)PFMSCAN_NSTRUCT : (int)c1 >= nl);
                if (idx >= 0) {
                    if (idx < 64) f0 |= (unsigned long long)bad << idx;
                    else f1 |= (unsigned long long)bad << (idx - 64);
                }
                out |= (bad ? 0u : PAIR ? c1 | (c2 << 3) : c1) << (8 * j);
            }
            if (i < cs) mine[i] = out;                             // beyond: no code of a block of this width (4 i - sh >= need)
        }
        const unsigned long long wmask = m == 64 ? ~0ull : (1ull << m) - 1;
        for (int w = 0; w < OCC_FANIN; ++w) {
            const unsigned long long win = w ? (f0 >> w) | (f1 << (64 - w)) : f0;
            valid |= (uint32_t)((win & wmask) == 0) << w;          // w >= nw: code w + m - 1 >= need is marked
        }
        if (a.bcnt && blockIdx.y == 0) a.bcnt[gb] = __popc(valid);
    }
    __syncthreads();                                               // the last barrier
    if (gb >= a.n_blk) return;
    const uint8_t *cb = reinterpret_cast<const uint8_t *>(cw + threadIdx.x * cs) + sh;
    const int rs = nl * ls;                                        // doubles per table row
    double *out = a.bs + gb * a.n_q + qc;
    if (valid == 0) {                                              // no window with a term: +0.0 without walking the block
        for (int q = 0; q < nq; ++q) out[q] = 0.0;
        return;
    }
    for (int q = 0; q < nq; q += QN) {
        double sum[QN];
#pragma unroll
        for (int i = 0; i < QN; ++i) sum[i] = 0.0;
#pragma unroll 1
        for (int w = 0; w < OCC_FANIN; ++w) {
            const uint8_t *cp = cb + w;
            const double *row = lt + q;
            double t[QN];
            occ_cells<QN>(row + (int)(PAIR ? cp[0] & 7u : cp[0]) * ls, t);
#pragma unroll 4
            for (int k = 1; k < m; ++k) {                          // the letters ...
                row += rs;
                double c[QN];
                occ_cells<QN>(row + (int)(PAIR ? cp[k] & 7u : cp[k]) * ls, c);
#pragma unroll
                for (int i = 0; i < QN; ++i) t[i] = t[i] * c[i];
            }
            if constexpr (PAIR) {
                row = lt + q + 4 * ls;
#pragma unroll 4
                for (int k = 0; k < m; ++k) {                      // ... then the structure, continuing the same chain
                    double c[QN];
                    occ_cells<QN>(row + (int)(cp[k] >> 3) * ls, c);
                    row += rs;
#pragma unroll
                    for (int i = 0; i < QN; ++i) t[i] = t[i] * c[i];
                }
            }
            const bool has = (valid >> w) & 1u;
#pragma unroll
            for (int i = 0; i < QN; ++i) sum[i] = sum[i] + (has ? t[i] : 0.0);
        }
#pragma unroll
        for (int i = 0; i < QN; ++i)
            if (q + i < nq) out[q + i] = sum[i];
    }
}

__global__ __launch_bounds__(BLOCK) void k_occ_level1(const OccArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= a.n_grp * a.n_q) return;
    const int64_t gg = t / a.n_q;
    const int q = (int)(t - gg * a.n_q);
    const int64_t g = a.grp_base + gg;
    const int64_t r = occ_record(a.grp_start, a.r0, a.r1, g);
    const int64_t first = (g - a.grp_start[r]) * OCC_FANIN;        // first block of the group, within the record
    const int n = (int)min((int64_t)OCC_FANIN, a.blk_start[r + 1] - a.blk_start[r] - first);
    const int64_t b0 = a.blk_start[r] - a.blk_base + first;
    const double *in = a.bs + b0 * a.n_q + q;
    double s = in[0];
    for (int i = 1; i < n; ++i) s = s + in[(int64_t)i * a.n_q];
    a.gs[gg * a.n_q + q] = s;
    if (a.bcnt && q == 0) {
        int c = 0;
        for (int i = 0; i < n; ++i) c += a.bcnt[b0 + i];
        a.gcnt[gg] = c;
    }
}

__global__ __launch_bounds__(BLOCK) void k_occ_finish(const OccArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= (a.r1 - a.r0) * a.n_q) return;
    const int64_t rr = t / a.n_q;
    const int q = (int)(t - rr * a.n_q);
    const int64_t r = a.r0 + rr;
    const int64_t g0 = a.grp_start[r] - a.grp_base;
    int64_t n = a.grp_start[r + 1] - a.grp_start[r];
    double res = 0.0;                                              // n_win == 0
    if (n > 0) {
        double *x = a.gs + g0 * a.n_q + q;                         // element i at x[i * n_q]; level l + 1 overwrites the front of level l
        while (n > 1) {
            const int64_t no = (n + OCC_FANIN - 1) / OCC_FANIN;
            for (int64_t j = 0; j < no; ++j) {
                const int64_t c0 = j * OCC_FANIN, c1 = min(n, c0 + OCC_FANIN);
                double s = x[c0 * a.n_q];
                for (int64_t i = c0 + 1; i < c1; ++i) s = s + x[i * a.n_q];
                x[j * a.n_q] = s;                                  // j <= c0: read before it is overwritten, by this thread alone
            }
            n = no;
        }
        res = x[0];
    }
    const int x = a.q_first + q;                                   // the column; a cell of a motif is stored under a letter stride of 8
    a.occ[r * a.out_stride + (a.cell_nl ? x / a.cell_nl * 8 + x % a.cell_nl : x)] = res;
    if (a.windows && a.bcnt && q == 0) {
        int64_t c = 0;
        const int64_t ng = a.grp_start[r + 1] - a.grp_start[r];
        for (int64_t i = 0; i < ng; ++i) c += a.gcnt[g0 + i];
        a.windows[r] = c;
    }
}

// ---- level 0 on averaged-structure profiles (OCCP_*, occp_load, occp_cells, occp_marginal: pfmscan_occ.hpp) -----------------
// the record of every run of the pass, so that a workgroup of k_occ_profile_blocks finds its run with two round trips to memory
// instead of a bisection of ~17 dependent loads (which, at 8 workgroups per CU, was most of a single-motif call's time)
__global__ __launch_bounds__(BLOCK) void k_occ_run_records(const OccArgs a)
{
    const int64_t r = a.r0 + (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= a.r1) return;
    const int64_t u1 = a.run_start[r + 1] - a.run_base;
    for (int64_t u = a.run_start[r] - a.run_base; u < u1; ++u) a.run_rec[u] = r;
}

template <typename T, bool SEQ, int QN>
__global__ __launch_bounds__(BLOCK) void k_occ_profile_blocks(const OccArgs a, const double *__restrict__ stab, const double *__restrict__ ltab,
                                                              double *__restrict__ bs)
{
    constexpr int RB = 7 * (int)sizeof(T);                         // bytes of a row
    constexpr int PER = 16 / (int)sizeof(T);                       // cells of a vector
    __shared__ double rows[OCCP_ROWS * 7];
    __shared__ double tl[QN * OCCP_TS];
    __shared__ uint8_t cl[SEQ ? (OCCP_ROWS + 7) / 8 * 8 : 8];
    const int t = threadIdx.x, m = a.m;
    const int64_t u = a.run_base + blockIdx.x;                     // this workgroup's run
    const int64_t r = a.run_rec[blockIdx.x];
    const int64_t b0 = (u - a.run_start[r]) * OCCP_RUN;            // its first block, within the record
    const int64_t w0 = b0 * OCC_FANIN;
    const int64_t n_win = a.rec_len[r] - m + 1;                    // > w0: the run exists
    const int nw = (int)min((int64_t)OCCP_WIN, n_win - w0);
    const int nb = (nw + OCC_FANIN - 1) / OCC_FANIN;
    const int nrows = nw + m - 1;                                  // all inside the record: the separator is not among them
    const int64_t row0 = a.rec_off[r] + w0;
    {
        const int64_t first = row0 * RB, end = first + (int64_t)nrows * RB, base = first & ~(int64_t)15, total = a.n_pos * RB;
        const int shift = (int)(first - base) / (int)sizeof(T);
        const int ncell = nrows * 7, nvec = (int)((end - base + 15) / 16);
        for (int v = t; v < nvec; v += BLOCK) {
            double d[PER];
            occp_cells(occp_load(a.profile, base + (int64_t)v * 16, total), d, T());
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int idx = v * PER + j - shift;
                if (idx >= 0 && idx < ncell) rows[idx] = d[j];
            }
        }
        if constexpr (SEQ)
            for (int i = t; i < nrows; i += BLOCK) cl[i] = a.codes[row0 + i];
    }
    __syncthreads();
    const bool mine = t < nw;
    bool has = mine;                                               // this lane's window has a term
    if constexpr (SEQ) {
        if (mine)
            for (int k = 0; k < m; ++k) has = has && (cl[t + k] & 7u) < 4u;
    }
    const int64_t gb = a.blk_start[r] - a.blk_base + b0;           // the run's first block, within the pass
    if (a.bcnt && blockIdx.y == 0) {
        const unsigned long long bal = __ballot(has);
        const int lane = t & 63, b = 2 * (t >> 6) + (lane >> 5);
        if ((lane & 31) == 0 && b < nb) a.bcnt[gb + b] = __popcll(lane ? bal >> 32 : bal & 0xFFFFFFFFull);
    }
    const int qc = (int)blockIdx.y * OCCP_CHUNK;                   // first motif of this workgroup, within the pass
    const int nq = min(OCCP_CHUNK, a.n_q - qc);
    const int64_t ms = (int64_t)m * 7, ml = (int64_t)m * 8;
    for (int q = 0; q < nq; q += QN) {
        double tt[QN];
#pragma unroll
        for (int i = 0; i < QN; ++i) tt[i] = 0.0;
        if (mine) {
            const int64_t qg = (int64_t)a.q_first + qc + q;
            const double *rw = rows + t * 7;
            double x[7];
            if constexpr (SEQ) {
                int c = cl[t] & 7;
#pragma unroll
                for (int i = 0; i < QN; ++i) tt[i] = ltab[(qg + min(i, nq - 1 - q)) * ml + c];
                for (int k = 1; k < m; ++k) {
                    c = cl[t + k] & 7;
#pragma unroll
                    for (int i = 0; i < QN; ++i) tt[i] = tt[i] * ltab[(qg + min(i, nq - 1 - q)) * ml + k * 8 + c];
                }
            }
#pragma unroll
            for (int c = 0; c < 7; ++c) x[c] = rw[c];
#pragma unroll
            for (int i = 0; i < QN; ++i) {
                const double d = occp_marginal(x, stab + (qg + min(i, nq - 1 - q)) * ms);
                tt[i] = SEQ ? tt[i] * d : d;
            }
            for (int k = 1; k < m; ++k) {
                rw += 7;
#pragma unroll
                for (int c = 0; c < 7; ++c) x[c] = rw[c];
#pragma unroll
                for (int i = 0; i < QN; ++i) tt[i] = tt[i] * occp_marginal(x, stab + (qg + min(i, nq - 1 - q)) * ms + k * 7);
            }
        }
        if (q) __syncthreads();                                    // the adders of the last round are done with tl
#pragma unroll
        for (int i = 0; i < QN; ++i) tl[i * OCCP_TS + t + (t >> 5)] = has ? tt[i] : 0.0;
        __syncthreads();
        if (t < OCCP_RUN * QN) {
            const int i = t >> 3, b = t & 7;
            if (b < nb && q + i < nq) {
                const double *p = tl + i * OCCP_TS + b * (OCC_FANIN + 1);
                double v[OCC_FANIN];                               // all 32 reads in flight before the dependent additions
#pragma unroll
                for (int j = 0; j < OCC_FANIN; ++j) v[j] = p[j];
                double s = v[0];
#pragma unroll
                for (int j = 1; j < OCC_FANIN; ++j) s = s + v[j];  // the block padded with +0.0 to 32 (skipped windows are +0.0 too)
                bs[(gb + b) * a.n_q + qc + q + i] = n_win == 1 ? v[0] : s;   // a lone window is the record's sum as it is
            }
        }
    }
}

void occ_launch_run_records(const OccArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_occ_run_records, dim3((unsigned)((a.r1 - a.r0 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, a);
}

int occ_launch_upper(pfmscan_ctx *ctx, const OccArgs &a, hipStream_t st)
{
    hipError_t e;
    if (a.n_blk > 0) {
        hipLaunchKernelGGL(k_occ_level1, dim3((unsigned)((a.n_grp * a.n_q + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return fail_hip(ctx, e, "k_occ_level1");
    }
    hipLaunchKernelGGL(k_occ_finish, dim3((unsigned)(((a.r1 - a.r0) * a.n_q + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail_hip(ctx, e, "k_occ_finish");
    return PFMSCAN_OK;
}

int64_t occ_scratch_cap()
{
    if (const char *e = std::getenv("PFMSCAN_OCC_SCRATCH_DOUBLES")) return std::max<int64_t>(1, std::atoll(e));
    return OCC_SCRATCH_DOUBLES;
}

static int occ_qn(int nq) { return nq >= 8 ? 8 : nq >= 4 ? 4 : nq >= 2 ? 2 : 1; }


// motifs per LDS chunk: the most (up to n_q) whose padded tables fit OCC_LDS_DOUBLES; one motif always fits
static int occ_chunk(int m, int n_letters, int n_q)
{
    int c = std::max(1, std::min(n_q, OCC_LDS_DOUBLES / (m * n_letters)));
    while (c > 1 && m * n_letters * occ_ls(c, occ_qn(c)) > OCC_LDS_DOUBLES) --c;
    return c;
}

template <bool PAIR>
static hipError_t occ_launch_blocks(const OccArgs &a, hipStream_t st)
{
    const int qn = occ_qn(a.chunk), nl = PAIR ? OCC_PAIR_LETTERS : a.n_letters;
    const size_t lds = (size_t)BLOCK * occ_strip(a.m) * 4 + (size_t)a.m * nl * occ_ls(a.chunk, qn) * sizeof(double);
    const dim3 grid((unsigned)((a.n_blk + BLOCK - 1) / BLOCK), (unsigned)((a.n_q + a.chunk - 1) / a.chunk));
    if (qn == 8) hipLaunchKernelGGL((k_occ_blocks<8, PAIR>), grid, dim3(BLOCK), lds, st, a);
    else if (qn == 4) hipLaunchKernelGGL((k_occ_blocks<4, PAIR>), grid, dim3(BLOCK), lds, st, a);
    else if (qn == 2) hipLaunchKernelGGL((k_occ_blocks<2, PAIR>), grid, dim3(BLOCK), lds, st, a);
    else hipLaunchKernelGGL((k_occ_blocks<1, PAIR>), grid, dim3(BLOCK), lds, st, a);
    return hipGetLastError();
}

template <typename T, bool SEQ>
static void occ_launch_profile_qn(const OccArgs &a, int qn, const dim3 grid, const double *stab, hipStream_t st)
{
    if (qn == 8) hipLaunchKernelGGL((k_occ_profile_blocks<T, SEQ, 8>), grid, dim3(BLOCK), 0, st, a, stab, a.tables, a.bs);
    else if (qn == 4) hipLaunchKernelGGL((k_occ_profile_blocks<T, SEQ, 4>), grid, dim3(BLOCK), 0, st, a, stab, a.tables, a.bs);
    else if (qn == 2) hipLaunchKernelGGL((k_occ_profile_blocks<T, SEQ, 2>), grid, dim3(BLOCK), 0, st, a, stab, a.tables, a.bs);
    else hipLaunchKernelGGL((k_occ_profile_blocks<T, SEQ, 1>), grid, dim3(BLOCK), 0, st, a, stab, a.tables, a.bs);
}

static hipError_t occ_launch_profile(const OccArgs &a, int dtype, bool seq, int64_t n_run, const double *stab, hipStream_t st)
{
    const int qn = occ_qn(std::min(a.n_q, OCCP_CHUNK));
    const dim3 grid((unsigned)n_run, (unsigned)((a.n_q + OCCP_CHUNK - 1) / OCCP_CHUNK));
    if (dtype == PFMSCAN_PROFILE_F64) {
        if (seq) occ_launch_profile_qn<double, true>(a, qn, grid, stab, st);
        else occ_launch_profile_qn<double, false>(a, qn, grid, stab, st);
    } else {
        if (seq) occ_launch_profile_qn<float, true>(a, qn, grid, stab, st);
        else occ_launch_profile_qn<float, false>(a, qn, grid, stab, st);
    }
    return hipGetLastError();
}

// ---- the frame of a driver (pfmscan_occ.hpp) -------------------------------------------------------------------------------
int occ_upload_tables(pfmscan_ctx *ctx, const double *letter_tables, const double *struct_tables, size_t stab_bytes, int n_motifs, int m,
                      hipStream_t st, const double *&d_tab, const double *&d_stab)
{
    int rc;
    const size_t tab_bytes = letter_tables ? (size_t)n_motifs * m * 8 * sizeof(double) : 0;
    if (!struct_tables) stab_bytes = 0;
    if ((rc = ensure(ctx, ctx->occ_tab, tab_bytes + stab_bytes))) return rc;
    d_tab = tab_bytes ? (const double *)ctx->occ_tab.p : nullptr;
    d_stab = (const double *)((const unsigned char *)ctx->occ_tab.p + tab_bytes);
    if (tab_bytes && (rc = upload(ctx, ctx->occ_tab.p, letter_tables, tab_bytes, st))) return rc;
    if (stab_bytes && (rc = upload(ctx, (void *)d_stab, struct_tables, stab_bytes, st))) return rc;
    return PFMSCAN_OK;
}

int occ_frame(pfmscan_ctx *ctx, const OccPlan &p, int cells, const OccRecords &rec, int n_motifs, int m, int n_letters, hipStream_t st, OccArgs &a)
{
    int rc;
    const size_t per_blk = (size_t)p.n_u_max * cells * 8;          // bytes of a block's (a group's) sums
    if ((rc = ensure(ctx, ctx->occ_idx, (p.start.size() + (size_t)p.need_run) * 8))) return rc;   // the prefix tables, then a pass's run -> record
    if ((rc = ensure(ctx, ctx->occ_bs, std::max<size_t>((size_t)p.need_blk * per_blk, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->occ_gs, std::max<size_t>((size_t)p.need_grp * per_blk, 16)))) return rc;
    if ((rc = upload(ctx, ctx->occ_idx.p, p.start.data(), p.start.size() * 8, st))) return rc;
    a.n_pos = rec.n_pos;
    a.rec_off = rec.d_off;
    a.rec_len = rec.d_len;
    a.blk_start = (const int64_t *)ctx->occ_idx.p;
    a.grp_start = a.blk_start + rec.n_rec + 1;
    if (p.runs) {
        a.run_start = a.grp_start + rec.n_rec + 1;
        a.run_rec = (int64_t *)ctx->occ_idx.p + p.start.size();
    }
    a.m = m;
    a.n_letters = n_letters;
    a.n_motifs = n_motifs;
    a.bs = (double *)ctx->occ_bs.p;
    a.gs = (double *)ctx->occ_gs.p;
    return PFMSCAN_OK;
}

int64_t occ_set_pass(OccArgs &a, const OccPlan &p, size_t i)
{
    a.r0 = p.cuts[i];
    a.r1 = p.cuts[i + 1];
    a.blk_base = p.blk()[a.r0];
    a.n_blk = p.blk()[a.r1] - a.blk_base;
    a.grp_base = p.grp()[a.r0];
    a.n_grp = p.grp()[a.r1] - a.grp_base;
    a.run_base = p.runs ? p.run()[a.r0] : 0;
    return p.runs ? p.run()[a.r1] - a.run_base : 0;
}

int occ_run(pfmscan_ctx *ctx, const char *who, const double *ratio_tables, int n_motifs, int m, int n_letters, const uint8_t *d_codes,
            const OccRecords &rec, double *d_occ, int64_t *d_windows, hipStream_t st, const OccProfile *pf, const OccPair *pr)
{
    // motifs per pass: all of them unless the longest record's block sums alone pass the cap; then records per pass
    const OccPlan p = occ_plan(rec.len, rec.n_rec, m, n_motifs, 1, 1, occ_scratch_cap(), pf != nullptr);
    // a profile pass launches a workgroup per run, and has no more runs than blocks
    if ((p.need_blk + BLOCK - 1) / BLOCK > 0x7FFFFFFF || (pf && p.need_blk > 0x7FFFFFFF)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": a record is too long for one call");
    int rc;
    OccArgs a{};
    const double *d_stab;
    if ((rc = occ_upload_tables(ctx, ratio_tables, pf ? pf->struct_tables : pr ? pr->struct_tables : nullptr,
                                (size_t)n_motifs * m * (pf ? 7 : 8) * sizeof(double), n_motifs, m, st, a.tables, d_stab)))
        return rc;
    if ((rc = occ_frame(ctx, p, 1, rec, n_motifs, m, n_letters, st, a))) return rc;
    if ((rc = ensure(ctx, ctx->occ_cnt, std::max<size_t>((size_t)(p.need_blk + p.need_grp) * 4, 16)))) return rc;
    a.codes = d_codes;
    a.profile = pf ? (const unsigned char *)pf->d_profile : nullptr;
    a.codes2 = pr ? pr->d_codes2 : nullptr;
    a.tables2 = pr ? d_stab : nullptr;
    a.occ = d_occ;
    a.out_stride = n_motifs;
    a.windows = d_windows;
    const int n_q_max = (int)p.n_u_max;
    for (int q0 = 0; q0 < n_motifs; q0 += n_q_max) {
        a.q_first = q0;
        a.n_q = std::min(n_q_max, n_motifs - q0);
        a.chunk = pf ? OCCP_CHUNK : occ_chunk(m, pr ? OCC_PAIR_LETTERS : n_letters, a.n_q);
        if ((a.n_q + a.chunk - 1) / a.chunk > 65535) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many motifs for one call");
        const bool count = d_windows && q0 == 0;                   // Windows does not depend on the motif: counted in the first pass
        a.bcnt = count ? (int *)ctx->occ_cnt.p : nullptr;
        a.gcnt = count ? a.bcnt + p.need_blk : nullptr;
        for (size_t i = 0; i < p.n_pass(); ++i) {
            const int64_t n_run = occ_set_pass(a, p, i);
            if (a.n_blk > 0) {
                if (pf) occ_launch_run_records(a, st);
                const hipError_t e = pf ? occ_launch_profile(a, pf->dtype, ratio_tables != nullptr, n_run, d_stab, st)
                                     : pr ? occ_launch_blocks<true>(a, st) : occ_launch_blocks<false>(a, st);
                if (e != hipSuccess) return fail_hip(ctx, e, pf ? "k_occ_profile_blocks" : "k_occ_blocks");
            }
            if ((rc = occ_launch_upper(ctx, a, st))) return rc;
        }
    }
    return PFMSCAN_OK;
}

// ---- the pieces of the entry points (pfmscan_occ.hpp) ----------------------------------------------------------------------
int occ_check_base(pfmscan_ctx *ctx, const char *who, int m, const char *own, int n_motifs, int64_t n_rec, int64_t n_pos, const char *missing)
{
    if (m < 1 || m > PFMSCAN_MAX_M)
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": width " + std::to_string(m) + " outside 1 .. PFMSCAN_MAX_M (" + std::to_string(PFMSCAN_MAX_M) + ")");
    if (own) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + own);
    if (n_motifs < 0 || n_rec < 0 || n_pos < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": negative size");
    if (n_motifs > 0 && missing) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + missing);
    return PFMSCAN_OK;
}

int occ_check(pfmscan_ctx *ctx, const char *who, const double *ratio_tables, int n_motifs, int m, int n_letters, int64_t n_pos, int64_t n_rec)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    return occ_check_base(ctx, who, m, n_letters != 4 && n_letters != PFMSCAN_NSTRUCT ? ": n_letters must be 4 or 7" : nullptr, n_motifs, n_rec, n_pos,
                          ratio_tables ? nullptr : ": ratio_tables is NULL");
}

int occ_pair_check(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int64_t n_pos,
                   int64_t n_rec)
{
    return occ_check_base(ctx, who, m, nullptr, n_motifs, n_rec, n_pos, seq_tables && struct_tables ? nullptr : ": seq_tables or struct_tables is NULL");
}

// the checks both profile entry points share
static int occp_check(pfmscan_ctx *ctx, const char *who, const double *struct_tables, int n_motifs, int m, int profile_dtype, int64_t n_pos,
                      int64_t n_rec)
{
    const bool dtype_ok = profile_dtype == PFMSCAN_PROFILE_F32 || profile_dtype == PFMSCAN_PROFILE_F64;
    return occ_check_base(ctx, who, m, dtype_ok ? nullptr : ": profile_dtype must be PFMSCAN_PROFILE_F32 or F64", n_motifs, n_rec, n_pos,
                          struct_tables ? nullptr : ": struct_tables is NULL");
}

// ascending, disjoint, inside [0, n_pos)
static int occ_check_records(pfmscan_ctx *ctx, const char *who, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, int64_t n_pos)
{
    int64_t end = 0;
    for (int64_t r = 0; r < n_rec; ++r) {
        if (rec_len[r] < 0 || rec_off[r] < end || rec_len[r] > n_pos - rec_off[r])
            return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": record " + std::to_string(r) + " does not ascend or leaves the stream");
        end = rec_off[r] + rec_len[r];
    }
    return PFMSCAN_OK;
}

int occ_records_home(pfmscan_ctx *ctx, const char *who, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, int64_t n_pos,
                     std::vector<int64_t> &host, OccRecords &rec)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    host.resize(2 * (size_t)n_rec);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), d_rec_off, (size_t)n_rec * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(host.data() + n_rec, d_rec_len, (size_t)n_rec * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rec = OccRecords{host.data(), host.data() + n_rec, d_rec_off, d_rec_len, n_rec, n_pos};
    return occ_check_records(ctx, who, rec.off, rec.len, n_rec, n_pos);
}

int occ_records_up(pfmscan_ctx *ctx, const char *who, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, OccRecords &rec)
{
    int rc;
    if ((rc = occ_check_records(ctx, who, rec_off, rec_len, n_rec, ctx->staged_n))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->occ_rec, (size_t)n_rec * 16))) return rc;
    int64_t *d_off = (int64_t *)ctx->occ_rec.p, *d_len = d_off + n_rec;
    if ((rc = upload(ctx, d_off, rec_off, (size_t)n_rec * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d_len, rec_len, (size_t)n_rec * 8, ctx->stream))) return rc;
    rec = OccRecords{rec_off, rec_len, d_off, d_len, n_rec, ctx->staged_n};
    return PFMSCAN_OK;
}

int occ_copy_home(pfmscan_ctx *ctx, std::initializer_list<OccHome> arrays)
{
    for (const OccHome &h : arrays)
        if (h.dst) HIP_TRY(ctx, hipMemcpyAsync(h.dst, h.d_src, h.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFMSCAN_OK;
}

// The three _staged forms after their own tests of what is staged and of the arguments: the records go up, the outputs are
// carved from ctx->occ_out, run(rec, d_occ, d_windows) launches on ctx->stream, the outputs come home.
template <typename Run>
static int occ_staged(pfmscan_ctx *ctx, const char *who, int n_motifs, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *occ,
                      int64_t *windows, Run run)
{
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len || !occ) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or output");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const size_t cells = (size_t)n_rec * n_motifs;
    if ((rc = ensure(ctx, ctx->occ_out, cells * 8 + (size_t)n_rec * 8))) return rc;
    double *d_occ = (double *)ctx->occ_out.p;
    int64_t *d_win = windows ? (int64_t *)(d_occ + cells) : nullptr;
    if ((rc = run(rec, d_occ, d_win))) return rc;
    return occ_copy_home(ctx, {{occ, d_occ, cells * 8}, {windows, d_win, (size_t)n_rec * 8}});
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_occupancy_dev(pfmscan_ctx *ctx, const double *ratio_tables, int n_motifs, int m, int n_letters, const uint8_t *d_codes,
                          int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_occ,
                          int64_t *d_windows)
{
    const char *who = "pfmscan_occupancy_dev";
    if (int rc = occ_check(ctx, who, ratio_tables, n_motifs, m, n_letters, n_pos, n_rec)) return rc;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || !d_occ || (n_pos > 0 && !d_codes)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table, codes or output");
    if (misaligned(d_codes)) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    return occ_run(ctx, who, ratio_tables, n_motifs, m, n_letters, d_codes, rec, d_occ, d_windows, ctx->stream);
}

int pfmscan_occupancy_staged(pfmscan_ctx *ctx, int which, const double *ratio_tables, int n_motifs, int m, int n_letters,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *occ, int64_t *windows)
{
    const char *who = "pfmscan_occupancy_staged";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (which != 0 && which != 1) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": which must be 0 (codes) or 1 (codes2)");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && !(which ? ctx->staged_codes2 : ctx->staged_codes))
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + (which ? ": no codes2 are staged (pfmscan_stage_codes2)" : ": no codes are staged"));
    if (int rc = occ_check(ctx, who, ratio_tables, n_motifs, m, n_letters, ctx->staged_n, n_rec)) return rc;
    const uint8_t *d_codes = (const uint8_t *)(which ? ctx->codes2.p : ctx->codes.p);
    return occ_staged(ctx, who, n_motifs, rec_off, rec_len, n_rec, occ, windows, [&](const OccRecords &rec, double *d_occ, int64_t *d_win) {
        return occ_run(ctx, who, ratio_tables, n_motifs, m, n_letters, d_codes, rec, d_occ, d_win, ctx->stream);
    });
}

int pfmscan_occupancy_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                  const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                  const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_occ, int64_t *d_windows)
{
    const char *who = "pfmscan_occupancy_profile_dev";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = occp_check(ctx, who, struct_tables, n_motifs, m, profile_dtype, n_pos, n_rec)) return rc;
    if (seq_tables && !d_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": seq_tables (joint mode) needs the codes");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || !d_occ || (n_pos > 0 && !d_profile)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table, profile or output");
    if (misaligned(d_profile) || (seq_tables && misaligned(d_codes)))
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    const OccProfile pf{struct_tables, d_profile, profile_dtype};
    return occ_run(ctx, who, seq_tables, n_motifs, m, 4, seq_tables ? d_codes : nullptr, rec, d_occ, d_windows, ctx->stream, &pf);
}

int pfmscan_occupancy_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                     const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *occ, int64_t *windows)
{
    const char *who = "pfmscan_occupancy_profile_staged";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (!ctx->staged_profile) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no profile is staged");
    if (seq_tables && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": seq_tables (joint mode) needs staged codes");
    if (int rc = occp_check(ctx, who, struct_tables, n_motifs, m, ctx->staged_dtype, ctx->staged_n, n_rec)) return rc;
    const OccProfile pf{struct_tables, ctx->profile.p, ctx->staged_dtype};
    const uint8_t *d_codes = seq_tables ? (const uint8_t *)ctx->codes.p : nullptr;
    return occ_staged(ctx, who, n_motifs, rec_off, rec_len, n_rec, occ, windows, [&](const OccRecords &rec, double *d_occ, int64_t *d_win) {
        return occ_run(ctx, who, seq_tables, n_motifs, m, 4, d_codes, rec, d_occ, d_win, ctx->stream, &pf);
    });
}

int pfmscan_occupancy_pair_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                               const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                               const int64_t *d_rec_len, int64_t n_rec, double *d_occ, int64_t *d_windows)
{
    const char *who = "pfmscan_occupancy_pair_dev";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = occ_pair_check(ctx, who, seq_tables, struct_tables, n_motifs, m, n_pos, n_rec)) return rc;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || !d_occ || (n_pos > 0 && (!d_codes || !d_codes2)))
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table, codes or output");
    if (misaligned(d_codes) || misaligned(d_codes2)) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    const OccPair pr{struct_tables, d_codes2};
    return occ_run(ctx, who, seq_tables, n_motifs, m, 4, d_codes, rec, d_occ, d_windows, ctx->stream, nullptr, &pr);
}

int pfmscan_occupancy_pair_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                  const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *occ, int64_t *windows)
{
    const char *who = "pfmscan_occupancy_pair_staged";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes are staged");
    if (ctx->staged_n > 0 && !ctx->staged_codes2) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes2 are staged (pfmscan_stage_codes2)");
    if (int rc = occ_pair_check(ctx, who, seq_tables, struct_tables, n_motifs, m, ctx->staged_n, n_rec)) return rc;
    const OccPair pr{struct_tables, (const uint8_t *)ctx->codes2.p};
    return occ_staged(ctx, who, n_motifs, rec_off, rec_len, n_rec, occ, windows, [&](const OccRecords &rec, double *d_occ, int64_t *d_win) {
        return occ_run(ctx, who, seq_tables, n_motifs, m, 4, (const uint8_t *)ctx->codes.p, rec, d_occ, d_win, ctx->stream, nullptr, &pr);
    });
}

}  // extern "C"
