// pfmscan_expect_profile.hip -- expected counts on averaged-structure profiles: weighted ROW sums (DESIGN.md 5i,
// include/pfmscan.h "expected counts on averaged-structure profiles").
//
// Per record and motif the matrix exp_struct [m][8]: cell [k][c], c < 7 in the profile's STORED column order, is the sum over
// the record's windows of x_s = has_s ? w_s * r[s + k][c] : +0.0 -- one rounded product each, float rows widened first -- in
// the occupancy's left-aligned tree of fan-in 32 anchored at the record's first window; column 7 is +0.0.  Optionally
// exp_seq [m][8], the cell of pfmscan_expect.hip with this call's weights: x_s = (has_s && (codes[s + k] & 7) == c) ? w_s :
// +0.0, c < 4.  The term t_s of a window and whether it has one come from the tables that are given:
//   struct_tables only   the structure-only chain of marginals of k_occ_profile_blocks; every window has a term
//   both                 its joint chain: the letters, then m marginals; a window with a code >= 4 has no term
//   seq_tables only      the letter chain of k_occ_blocks / k_exp_blocks over the 4 RNA letters
// and the weight is the term (PFMSCAN_EXPECT_RATIO) or t_s * v, v = 1.0 / occ_r (PFMSCAN_EXPECT_POSTERIOR; occ_r == 0.0: every
// weight +0.0).  occ_r is what pfmscan_occupancy_profile_* / pfmscan_occupancy_* give for the same tables: the call runs that
// code first (occ_run, with the profile or without) and k_exp_inverse over its result.  The marginal has one definition
// (occp_marginal, pfmscan_occ.hpp).  No transcendental, no atomics, no tolerance: tests/expect_profile_rules.py restates it
// in numpy and the bits are compared.
//
//   k_expp_blocks<T, ST, SEQ>   level 0, on k_occ_profile_blocks' plan.  A workgroup of 256 lanes owns a run of 8 consecutive
//                   blocks of one record (256 windows).  The run's nw + m - 1 rows are fetched as the aligned 16-byte vectors
//                   that cover them (the stream's last one cut short) and parked in LDS as doubles, the codes beside them
//                   where a sequence table is given.  Per motif a lane makes its window's term and weight and parks the
//                   weight (+0.0 for a window without a term) one double apart per block; a ballot leaves which windows have
//                   a term.  Then a lane per (block, column k) walks the block's 32 windows in order: it reads a weight once
//                   and the 7 cells of row i + k, and advances 7 sums held in registers named at compile time (the loop over
//                   the windows is unrolled; four windows' 4 + 28 reads are in flight before their dependent additions).
//                   The first product is copied, not added to zero; a block is padded to 32 with +0.0; a lone window is the
//                   record's sum as it is.  exp_seq's 4 sums per (block, column) follow in a second walk, by the same
//                   tree.  One writer per scratch cell.
//                   The row image is padded by 4 doubles per 32 rows (EXPP_PAD below: without it the adders of the 8 blocks
//                   read one bank, 8 ways; measured 23.3 -> 16.1 ms per call at w = 8, profiles/expect_profile/NOTES.md).
//                   Static LDS 20 304 bytes (rows 18 160, weights 2 112, masks 32), 20 624 with the codes (320);
//                   VGPRs 122 (structure only), 130 (joint), 125 (sequence only), the same for float and double rows;
//                   no scratch, no spills, no register indexed at run time.  The adders are 8 m items per motif: with one
//                   motif of w = 8 one of the four waves adds while three wait at the barrier (a measured limit, NOTES.md).
//   k_expp_blocks<T, ST, true, JOINT = true>   the same kernel with the nucleotide x context table of a matrix row (include/pfmscan.h
//                   "The expected nucleotide x context table"): exp_joint [m][4][8], cell [k][a][c] the sum of
//                   x_s = (has_s && (codes[s + k] & 7) == a) ? w_s * r[s + k][c] : +0.0 -- exp_struct's product, one more
//                   condition in its select.  After the walks above a lane per (block, k, a) walks the block's 32 windows with
//                   expp_step's scheme (four windows' weight, code and 7 cells in flight, 7 sums in registers named at compile
//                   time): 32 m items per motif where the structure adders have 8 m, so w = 8 fills all four waves.  The four
//                   lanes of a (block, k) read the same LDS addresses (broadcasts); no new LDS array.  With JOINT any of the
//                   three scratch regions may be null (the entry points with the table leave any output out).  Calls without
//                   the table launch the instantiations without JOINT, whose gfx950 code is instruction for instruction what
//                   it was before the parameter existed (ExppArgs grew at its END).
//                   VGPRs / SGPRs / static LDS: <T, true, false> 122 / 63 / 20 304; <T, true, true> 130 / 79 / 20 624;
//                   <T, false, true> 125 / 65 / 20 624 (unchanged); <T, true, true, true> 143 / 84 / 20 624;
//                   <T, false, true, true> 138 / 70 / 20 624; the same for float and double rows; no scratch, no spills.
//                   143 VGPRs leave the 3 workgroups per CU that 130 leave (512 / 144 = 3 waves per SIMD).
//                   The other shape (a lane per (block, k) that makes each product once and selects into 28 register sums,
//                   56 VGPRs of sums) was NOT TRIED: this one did not disappoint (profiles/expect_profile_joint/NOTES.md).
// The rules pad EVERY level of the tree with +0.0, k_occ_level1 / k_occ_finish add the children that exist.  The two differ
// only in the sign of a zero: a sum whose values are all -0.0 stays -0.0 exactly where nothing is padded, i.e. when n_win is a
// power of 32.  The occupancy's terms are never -0.0; w * (-0.0) here can be.  Level 0 therefore adds the +0.0 of the padding
// itself (s + 0.0, which changes no other value) whenever n_win is not a power of 32.
// Levels 1 and up are occ_launch_upper, once over the structure matrix (cell_nl = 7), once over the sequence matrix
// (cell_nl = 4) and once over the table (a matrix of 4 m rows, cell_nl = 7, q_first = u_first * 28), each with its own scratch
// region in that order.  A call with the table plans as pfmscan_expect_pair_joint_* does (fill_blk, unit_group = m).  Scratch is bounded by occ_scratch_cap(): records run in passes, and when
// the longest record alone passes the cap, so do the matrix rows (motif, k) -- the 7 + 4 cells of a row stay together -- and
// with them the motifs: occ_plan (pfmscan_occ_plan.hpp) over matrix rows, on the frame of pfmscan_occ.hpp.
#include <algorithm>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_occ.hpp"

#pragma clang fp contract(off)   // products and sums are rounded one operation at a time: never an FMA

namespace pfmscan {

constexpr int EXPP_WS = OCC_FANIN + 1;                             // doubles between the weights of two blocks
constexpr int EXPP_STEP = 4;                                       // windows whose reads are in flight together
static_assert(OCC_FANIN % EXPP_STEP == 0, "whole steps");
// Row x of the run lies at double x * 7 + (x / 32) * EXPP_PAD of the LDS image.  Unpadded, 32 rows are 448 dwords = 7 times
// the 64 banks: the adder lanes of the 8 blocks (same column, same step) would all read one bank, 8 ways.  With 4 doubles
// between blocks the 8 blocks x 4 columns of a half-wave fall on 32 different bank pairs (the term's walk, 32 consecutive rows
// per half-wave, then meets one 2-way conflict where it crosses a block).
constexpr int EXPP_PAD = 4;
constexpr int EXPP_NJ = 4 * PFMSCAN_NSTRUCT;                       // cells of the table of a matrix row
constexpr int EXPP_FILL_ROUNDS = 16;                               // workgroups per CU a pass with the table should have (3 are resident)
constexpr int EXPP_ROWS_LDS = (OCCP_ROWS * 7 + (OCCP_ROWS - 1) / OCC_FANIN * EXPP_PAD + 1) / 2 * 2;
__device__ __forceinline__ int expp_row(int x) { return x * 7 + (x >> 5) * EXPP_PAD; }

struct ExppArgs {
    const double *stab;          // [n_motifs][m][7] device, or null
    const double *occ, *inv;     // [n_rec][n_motifs]: posterior mode, else null
    double *bs_struct;           // [n_blk][n_u * 7]
    double *bs_seq;              // [n_blk][n_u * 4] or null
    int u_first, n_u;            // matrix rows of the pass: u = motif * m + k
    double *bs_joint;            // [n_blk][n_u * 28]: column (u * 4 + a) * 7 + c; null without JOINT or when the table is not asked for.  Last: the
                                 // kernels without the table read the arguments they read before it existed
};

// n is 1, 32, 1024, ...: the tree over n values pads nowhere
__device__ __forceinline__ bool expp_pow32(int64_t n) { return (n & (n - 1)) == 0 && (__ffsll((long long)n) - 1) % 5 == 0; }

// one step of the 7 sums of a (block, column): EXPP_STEP windows from wp[0] and row x0 of the image; bit j of hm: window j of
// the step has a term.  All of the step's 4 + 28 reads are issued before the dependent additions.
// SEL (the table): a window counts only where the code under its column, cp[j], is nucleotide na; the codes are read with the rest.
template <bool FULL, bool FIRST, bool SEL = false>
__device__ __forceinline__ void expp_step(const double *__restrict__ wp, const double *__restrict__ rows, int x0, uint32_t hm, double (&s)[7],
                                          const uint8_t *__restrict__ cp = nullptr, int na = 0)
{
    double w[EXPP_STEP], x[EXPP_STEP][7];
    int code[EXPP_STEP];
#pragma unroll
    for (int j = 0; j < EXPP_STEP; ++j) {
        w[j] = wp[j];
        if constexpr (SEL) code[j] = cp[j] & 7;
        const double *rp = rows + expp_row(x0 + j);
#pragma unroll
        for (int c = 0; c < 7; ++c) x[j][c] = rp[c];
    }
#pragma unroll
    for (int j = 0; j < EXPP_STEP; ++j) {
        bool on = FULL || ((hm >> j) & 1u);
        if constexpr (SEL) on = on && code[j] == na;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const double v = on ? w[j] * x[j][c] : 0.0;
            if (FIRST && j == 0) s[c] = v;                         // the first value of a block is copied
            else s[c] = s[c] + v;
        }
    }
}

// the 7 sums of one (block, column): weights wp[0 .. 31], rows x0 + i of the image, bit i of hm: window i has a term
template <bool FULL>
__device__ __forceinline__ void expp_add(const double *__restrict__ wp, const double *__restrict__ rows, int x0, uint32_t hm, double (&s)[7])
{
    expp_step<FULL, true>(wp, rows, x0, hm, s);
#pragma unroll 1
    for (int i0 = EXPP_STEP; i0 < OCC_FANIN; i0 += EXPP_STEP) expp_step<FULL, false>(wp + i0, rows, x0 + i0, hm >> i0, s);
}

// the 7 sums of one (block, column, nucleotide) of the table: expp_add over the windows whose code cp[i] is na
template <bool FULL>
__device__ __forceinline__ void expp_add_sel(const double *__restrict__ wp, const double *__restrict__ rows, int x0, uint32_t hm, double (&s)[7],
                                             const uint8_t *__restrict__ cp, int na)
{
    expp_step<FULL, true, true>(wp, rows, x0, hm, s, cp, na);
#pragma unroll 1
    for (int i0 = EXPP_STEP; i0 < OCC_FANIN; i0 += EXPP_STEP) expp_step<FULL, false, true>(wp + i0, rows, x0 + i0, hm >> i0, s, cp + i0, na);
}

template <typename T, bool ST, bool SEQ, bool JOINT = false>
__global__ __launch_bounds__(BLOCK) void k_expp_blocks(const OccArgs a, const ExppArgs e)
{
    static_assert(!JOINT || SEQ, "the table reads the codes");
    constexpr int RB = 7 * (int)sizeof(T);                         // bytes of a row
    constexpr int PER = 16 / (int)sizeof(T);                       // cells of a vector
    __shared__ double rows[EXPP_ROWS_LDS];
    __shared__ double wl[OCCP_RUN * EXPP_WS];
    __shared__ uint8_t cl[(OCCP_ROWS + 7) / 8 * 8];
    __shared__ uint32_t hml[OCCP_RUN];
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
                if (idx >= 0 && idx < ncell) rows[idx + idx / (7 * OCC_FANIN) * EXPP_PAD] = d[j];
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
    {
        const unsigned long long bal = __ballot(has);
        const int lane = t & 63;
        if ((lane & 31) == 0) hml[2 * (t >> 6) + (lane >> 5)] = (uint32_t)(lane ? bal >> 32 : bal & 0xFFFFFFFFull);
    }
    const int64_t gb = a.blk_start[r] - a.blk_base + b0;           // the run's first block, within the pass
    const bool lone = n_win == 1, padded = !expp_pow32(n_win);
    const int64_t ms = (int64_t)m * 7, ml = (int64_t)m * 8;
    const int64_t ss = (int64_t)e.n_u * 7, sq = (int64_t)e.n_u * 4;   // doubles per block of the two scratch regions
    const int u_lo = e.u_first, u_hi = e.u_first + e.n_u;
    const int q_lo = u_lo / m;
    for (int q = q_lo; q * m < u_hi; ++q) {
        double wt = 0.0;
        if (has) {
            double tt = 0.0;
            if constexpr (SEQ) {
                const double *lt = a.tables + q * ml;
                tt = lt[cl[t] & 7];
                for (int k = 1; k < m; ++k) tt = tt * lt[k * 8 + (cl[t + k] & 7)];
            }
            if constexpr (ST) {
                const double *sp = e.stab + q * ms;
                double x[7];
                const double *rw = rows + expp_row(t);
#pragma unroll
                for (int c = 0; c < 7; ++c) x[c] = rw[c];
                const double d = occp_marginal(x, sp);
                tt = SEQ ? tt * d : d;
                for (int k = 1; k < m; ++k) {
                    rw = rows + expp_row(t + k);
#pragma unroll
                    for (int c = 0; c < 7; ++c) x[c] = rw[c];
                    tt = tt * occp_marginal(x, sp + k * 7);
                }
            }
            if (e.inv) {
                const int64_t p = r * a.n_motifs + q;
                tt = e.occ[p] == 0.0 ? 0.0 : tt * e.inv[p];
            }
            wt = tt;
        }
        if (q != q_lo) __syncthreads();                            // the adders of the last motif are done with wl
        wl[t + (t >> 5)] = wt;
        __syncthreads();                                           // also orders hml, written before the loop
        const int k_lo = max(u_lo - q * m, 0), k_hi = min(u_hi - q * m, m);
        const int items = (k_hi - k_lo) * OCCP_RUN;
        for (int it = t; it < ((!JOINT || e.bs_struct) ? items : 0); it += BLOCK) {   // with JOINT any of the three regions may be null
            const int b = it & (OCCP_RUN - 1), k = k_lo + (it >> 3);
            if (b >= nb) continue;
            const double *wp = wl + b * EXPP_WS;
            const int x0 = b * OCC_FANIN + k;                      // the row under column k of the block's first window
            const uint32_t hm = hml[b];
            double s[7];
            if (lone) {                                            // a lone window is the record's sum as it is
                const double w = wp[0];
                const double *rp = rows + expp_row(x0);
#pragma unroll
                for (int c = 0; c < 7; ++c) s[c] = (hm & 1u) ? w * rp[c] : 0.0;
            } else {
                if (hm == 0xFFFFFFFFu) expp_add<true>(wp, rows, x0, hm, s);
                else expp_add<false>(wp, rows, x0, hm, s);
                if (padded) {
#pragma unroll
                    for (int c = 0; c < 7; ++c) s[c] = s[c] + 0.0;  // the +0.0 a level above pads with (see the header)
                }
            }
            double *o = e.bs_struct + (gb + b) * ss + (int64_t)(q * m + k - u_lo) * 7;
#pragma unroll
            for (int c = 0; c < 7; ++c) o[c] = s[c];
        }
        if constexpr (SEQ) {
            if (e.bs_seq) {
                for (int it = t; it < items; it += BLOCK) {
                    const int b = it & (OCCP_RUN - 1), k = k_lo + (it >> 3);
                    if (b >= nb) continue;
                    const double *wp = wl + b * EXPP_WS;
                    const uint8_t *cp = cl + b * OCC_FANIN + k;
                    // the tree of exp_struct: the first value copied, the block padded with +0.0, a lone window as it is.
                    // (k_exp_blocks starts from 0.0 +, which gives the same bits unless a weight is -0.0 -- no table of
                    // the contract makes one; a negative profile cell in joint mode can)
                    const int f = cp[0] & 7;
                    const double w0 = wp[0];                       // +0.0 for a window without a term or beyond the record
                    double s0 = f == 0 ? w0 : 0.0, s1 = f == 1 ? w0 : 0.0, s2 = f == 2 ? w0 : 0.0, s3 = f == 3 ? w0 : 0.0;
                    if (!lone) {
#pragma unroll 8
                        for (int i = 1; i < OCC_FANIN; ++i) {
                            const int c = cp[i] & 7;
                            const double w = wp[i];
                            s0 = s0 + (c == 0 ? w : 0.0);
                            s1 = s1 + (c == 1 ? w : 0.0);
                            s2 = s2 + (c == 2 ? w : 0.0);
                            s3 = s3 + (c == 3 ? w : 0.0);
                        }
                        if (padded) {
                            s0 = s0 + 0.0;
                            s1 = s1 + 0.0;
                            s2 = s2 + 0.0;
                            s3 = s3 + 0.0;
                        }
                    }
                    double *o = e.bs_seq + (gb + b) * sq + (int64_t)(q * m + k - u_lo) * 4;
                    o[0] = s0;
                    o[1] = s1;
                    o[2] = s2;
                    o[3] = s3;
                }
            }
        }
        if constexpr (JOINT) {
            if (e.bs_joint) {
                // a lane per (block, column k, nucleotide na): exp_struct's walk with one more condition in the select.  The
                // four lanes of a (block, k) read the same weights, rows and codes (LDS broadcasts)
                for (int it = t; it < items * 4; it += BLOCK) {
                    const int b = it & (OCCP_RUN - 1), na = (it >> 3) & 3, k = k_lo + (it >> 5);
                    if (b >= nb) continue;
                    const double *wp = wl + b * EXPP_WS;
                    const int x0 = b * OCC_FANIN + k;
                    const uint8_t *cp = cl + x0;                   // the codes under column k of the block's windows
                    const uint32_t hm = hml[b];
                    double s[7];
                    if (lone) {
                        const double w = wp[0];
                        const double *rp = rows + expp_row(x0);
                        const bool on = (hm & 1u) && (cp[0] & 7) == na;
#pragma unroll
                        for (int c = 0; c < 7; ++c) s[c] = on ? w * rp[c] : 0.0;
                    } else {
                        if (hm == 0xFFFFFFFFu) expp_add_sel<true>(wp, rows, x0, hm, s, cp, na);
                        else expp_add_sel<false>(wp, rows, x0, hm, s, cp, na);
                        if (padded) {
#pragma unroll
                            for (int c = 0; c < 7; ++c) s[c] = s[c] + 0.0;
                        }
                    }
                    double *o = e.bs_joint + (gb + b) * ((int64_t)e.n_u * EXPP_NJ) + ((int64_t)(q * m + k - u_lo) * 4 + na) * 7;
#pragma unroll
                    for (int c = 0; c < 7; ++c) o[c] = s[c];
                }
            }
        }
    }
}

template <typename T>
static void expp_launch_t(const OccArgs &a, const ExppArgs &e, bool st_given, bool seq_given, bool table, const dim3 grid, hipStream_t st)
{
    if (table) {                                                   // seq_given: checked before anything is planned
        if (st_given) hipLaunchKernelGGL((k_expp_blocks<T, true, true, true>), grid, dim3(BLOCK), 0, st, a, e);
        else hipLaunchKernelGGL((k_expp_blocks<T, false, true, true>), grid, dim3(BLOCK), 0, st, a, e);
    } else if (st_given && seq_given) hipLaunchKernelGGL((k_expp_blocks<T, true, true>), grid, dim3(BLOCK), 0, st, a, e);
    else if (st_given) hipLaunchKernelGGL((k_expp_blocks<T, true, false>), grid, dim3(BLOCK), 0, st, a, e);
    else hipLaunchKernelGGL((k_expp_blocks<T, false, true>), grid, dim3(BLOCK), 0, st, a, e);
}

// Launches on st, does not wait.  d_exp_struct / d_exp_seq / d_exp_joint: at least one is not null; the entry points without the
// table always give d_exp_struct and never d_exp_joint, and run what they ran before it existed.
static int expp_run(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                    const uint8_t *d_codes, const void *d_profile, int dtype, const OccRecords &rec, double *d_exp_struct, double *d_exp_seq,
                    double *d_exp_joint, double *d_occ, int64_t *d_windows, hipStream_t st)
{
    int rc;
    const bool posterior = mode == PFMSCAN_EXPECT_POSTERIOR;
    const int64_t pairs = rec.n_rec * n_motifs;
    const int64_t n_unit = (int64_t)n_motifs * m;                  // matrix rows (motif, k)
    const int wide = d_exp_joint ? EXPP_NJ : 7;                    // columns of a matrix row in the widest matrix of the call
    if (n_unit * wide > (int64_t(1) << 30)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many motifs for one call");
    // the occupancy of the same records first: v of posterior mode, and what the caller asked for
    if (posterior || d_occ || d_windows) {
        if (!d_occ) {
            if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
            d_occ = (double *)ctx->exp_occ.p;
        }
        const OccProfile pf{struct_tables, d_profile, dtype};       // no structure tables: the occupancy of the letter strings
        if ((rc = occ_run(ctx, who, seq_tables, n_motifs, m, 4, seq_tables ? d_codes : nullptr, rec, d_occ, d_windows, st, struct_tables ? &pf : nullptr))) return rc;
    }
    ExppArgs e{};
    if (posterior) {
        if ((rc = ensure(ctx, ctx->exp_inv, (size_t)pairs * 8))) return rc;
        if ((rc = exp_launch_inverse(ctx, d_occ, (double *)ctx->exp_inv.p, pairs, st))) return rc;
        e.occ = d_occ;
        e.inv = (const double *)ctx->exp_inv.p;
    }
    // column 7 (4 .. 7) of every matrix row is +0.0; every other cell is written by k_occ_finish
    if (d_exp_struct) HIP_TRY(ctx, hipMemsetAsync(d_exp_struct, 0, (size_t)pairs * m * 8 * sizeof(double), st));
    if (d_exp_seq) HIP_TRY(ctx, hipMemsetAsync(d_exp_seq, 0, (size_t)pairs * m * 8 * sizeof(double), st));
    if (d_exp_joint) HIP_TRY(ctx, hipMemsetAsync(d_exp_joint, 0, (size_t)pairs * m * 4 * 8 * sizeof(double), st));
    // matrix rows per pass: all of them unless the longest record's block sums alone pass the cap; then records per pass
    const int nst = d_exp_struct ? 7 : 0, nsq = d_exp_seq ? 4 : 0;
    const int cells = nst + nsq + (d_exp_joint ? EXPP_NJ : 0);     // scratch doubles of a matrix row, all regions
    // with the table a matrix row takes up to 39 doubles of a block, and all rows of a library in a pass would leave room for a
    // few records only: a pass then holds whole motifs, as many as leave room for the blocks of a few rounds of workgroups
    const int64_t fill_blk = d_exp_joint ? (int64_t)EXPP_FILL_ROUNDS * std::max(ctx->n_cu, 1) * OCCP_RUN : 1;
    const OccPlan p = occ_plan(rec.len, rec.n_rec, m, n_unit, cells, wide, occ_scratch_cap(), true, fill_blk, d_exp_joint ? m : 1);
    if (p.need_blk > 0x7FFFFFFF) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": a record is too long for one call");   // a workgroup per run, no more runs than blocks
    OccArgs a{};
    if ((rc = occ_upload_tables(ctx, seq_tables, struct_tables, (size_t)n_motifs * m * 7 * sizeof(double), n_motifs, m, st, a.tables, e.stab))) return rc;
    if (!struct_tables) e.stab = nullptr;
    if ((rc = occ_frame(ctx, p, cells, rec, n_motifs, m, 4, st, a))) return rc;
    a.codes = seq_tables ? d_codes : nullptr;
    a.profile = (const unsigned char *)d_profile;
    a.out_stride = (int64_t)n_motifs * m * 8;
    // the scratch regions of a pass: the structure matrix's block and level-1 sums, then the sequence matrix's, then the table's
    double *bs_seq = a.bs + p.need_blk * p.n_u_max * nst, *gs_seq = a.gs + p.need_grp * p.n_u_max * nst;
    e.bs_struct = d_exp_struct ? a.bs : nullptr;
    e.bs_seq = d_exp_seq ? bs_seq : nullptr;
    e.bs_joint = d_exp_joint ? bs_seq + p.need_blk * p.n_u_max * nsq : nullptr;
    OccArgs aq = a;                                                // levels 1 and up of the sequence matrix
    OccArgs aj = a;                                                // and of the table: a matrix of 4 m rows (k, a) and 7 columns
    a.occ = d_exp_struct;
    a.cell_nl = 7;
    aq.bs = bs_seq;
    aq.gs = gs_seq;
    aq.occ = d_exp_seq;
    aq.cell_nl = 4;
    aj.bs = e.bs_joint;
    aj.gs = gs_seq + p.need_grp * p.n_u_max * nsq;
    aj.occ = d_exp_joint;
    aj.out_stride = a.out_stride * 4;
    aj.cell_nl = 7;
    // the kernels without the table always write the structure region: a call that leaves it out runs the table's kernel
    const bool table = d_exp_joint || !d_exp_struct;
    for (int64_t u0 = 0; u0 < n_unit; u0 += p.n_u_max) {
        e.u_first = (int)u0;
        e.n_u = (int)std::min<int64_t>(p.n_u_max, n_unit - u0);
        a.q_first = e.u_first * 7;
        a.n_q = e.n_u * 7;
        aq.q_first = e.u_first * 4;
        aq.n_q = e.n_u * 4;
        aj.q_first = e.u_first * EXPP_NJ;
        aj.n_q = e.n_u * EXPP_NJ;
        for (size_t i = 0; i < p.n_pass(); ++i) {
            const bool make_table = p.n_pass() > 1 || u0 == 0;     // one range of records: its table is made once, for all passes over the rows
            const int64_t n_run = occ_set_pass(a, p, i);
            occ_set_pass(aq, p, i);
            occ_set_pass(aj, p, i);
            if (a.n_blk > 0) {
                if (make_table) occ_launch_run_records(a, st);
                const dim3 grid((unsigned)n_run);
                if (dtype == PFMSCAN_PROFILE_F64) expp_launch_t<double>(a, e, struct_tables != nullptr, seq_tables != nullptr, table, grid, st);
                else expp_launch_t<float>(a, e, struct_tables != nullptr, seq_tables != nullptr, table, grid, st);
                hipError_t err = hipGetLastError();
                if (err != hipSuccess) return fail_hip(ctx, err, "k_expp_blocks");
            }
            if (d_exp_struct && (rc = occ_launch_upper(ctx, a, st))) return rc;
            if (d_exp_seq && (rc = occ_launch_upper(ctx, aq, st))) return rc;
            if (d_exp_joint && (rc = occ_launch_upper(ctx, aj, st))) return rc;
        }
    }
    return PFMSCAN_OK;
}

// the checks the entry points share, before the rule "n_rec == 0 or n_motifs == 0: nothing to do"
static int expp_check(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                      int profile_dtype, int64_t n_pos, int64_t n_rec, bool with_exp_seq, bool with_exp_joint)
{
    const char *own = profile_dtype != PFMSCAN_PROFILE_F32 && profile_dtype != PFMSCAN_PROFILE_F64 ? ": profile_dtype must be PFMSCAN_PROFILE_F32 or F64"
                      : mode != PFMSCAN_EXPECT_RATIO && mode != PFMSCAN_EXPECT_POSTERIOR       ? ": mode must be PFMSCAN_EXPECT_RATIO or PFMSCAN_EXPECT_POSTERIOR"
                                                                                               : nullptr;
    if (int rc = occ_check_base(ctx, who, m, own, n_motifs, n_rec, n_pos, nullptr)) return rc;
    if (!struct_tables && !seq_tables) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": struct_tables and seq_tables are both NULL");
    if (with_exp_seq && !seq_tables) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": exp_seq needs seq_tables");
    if (with_exp_joint && !seq_tables) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": exp_joint needs seq_tables (the table reads the codes)");
    return PFMSCAN_OK;
}

// the _dev form.  table: the form has a d_exp_joint (null there: the table is not asked for) and any output may be null
static int expect_profile_dev_any(pfmscan_ctx *ctx, const char *who, bool table, const double *struct_tables, const double *seq_tables, int n_motifs,
                                  int m, int mode, const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos,
                                  const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_exp_struct, double *d_exp_seq,
                                  double *d_exp_joint, double *d_occ, int64_t *d_windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = expp_check(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, profile_dtype, n_pos, n_rec, d_exp_seq != nullptr, d_exp_joint != nullptr))
        return rc;
    if (seq_tables && !d_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": seq_tables needs the codes");
    if (table && !d_exp_struct && !d_exp_seq && !d_exp_joint)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": d_exp_struct, d_exp_seq and d_exp_joint are all NULL");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || (!table && !d_exp_struct) || (n_pos > 0 && !d_profile))
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table, profile or output");
    if (misaligned(d_profile) || (seq_tables && misaligned(d_codes)))
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    return expp_run(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, d_codes, d_profile, profile_dtype, rec, d_exp_struct, d_exp_seq,
                    d_exp_joint, d_occ, d_windows, ctx->stream);
}

// the outputs of a _staged form: the matrices on the HOST (exp), or with merged their accumulators and verdicts; [0] structure,
// [1] sequence, [2] the table (table: the form has one and any output may be null; null there: not asked for)
struct ExppOut {
    double *exp[3];
    uint64_t *acc[3];
    int64_t *bad[3];
    bool merged, table;
};

// all _staged forms.  merged: the sums of the matrices over the records come home (acc, bad) instead of the matrices
static int expect_profile_staged_any(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                     int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const ExppOut &o, double *occ,
                                     int64_t *windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (!ctx->staged_profile) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no profile is staged");
    if (seq_tables && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": seq_tables needs staged codes");
    bool want[3];
    for (int i = 0; i < 3; ++i) want[i] = o.merged ? o.acc[i] != nullptr : o.exp[i] != nullptr;
    if (int rc = expp_check(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, ctx->staged_dtype, ctx->staged_n, n_rec, want[1], want[2])) return rc;
    if (o.table && !want[0] && !want[1] && !want[2])
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + (o.merged ? ": acc_struct, acc_seq and acc_joint are all NULL" : ": exp_struct, exp_seq and exp_joint are all NULL"));
    if (o.table && o.merged)
        for (int i = 0; i < 3; ++i)
            if (want[i] && !o.bad[i]) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": an accumulator without its bad");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len || (!o.table && (o.merged ? !o.acc[0] || !o.bad[0] || (want[1] && !o.bad[1]) : !o.exp[0])))
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or output");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const size_t pairs = (size_t)n_rec * n_motifs, cells = pairs * m * 8, all = (want[2] ? 6 : 2) * cells;   // the table is four matrices wide
    if ((rc = ensure(ctx, ctx->exp_out, (all + pairs + (size_t)n_rec) * 8))) return rc;
    double *d_base = (double *)ctx->exp_out.p;
    double *d_st = want[0] ? d_base : nullptr;
    double *d_sq = want[1] ? d_base + cells : nullptr;
    double *d_jt = want[2] ? d_base + 2 * cells : nullptr;
    double *d_occ = occ ? d_base + all : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_base + all + pairs) : nullptr;
    if ((rc = expp_run(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, (const uint8_t *)ctx->codes.p, ctx->profile.p, ctx->staged_dtype, rec, d_st,
                       d_sq, d_jt, d_occ, d_win, ctx->stream)))
        return rc;
    if (o.merged) {
        const ExpMergeOut out[3] = {{d_st, o.acc[0], o.bad[0], m}, {d_sq, o.acc[1], o.bad[1], m}, {d_jt, o.acc[2], o.bad[2], 4 * m}};
        return exp_merge_home(ctx, who, out, o.table ? 3 : 2, n_rec, n_motifs, m, d_occ, occ, d_win, windows);
    }
    return occ_copy_home(ctx, {{o.exp[0], d_st, cells * 8}, {o.exp[1], d_sq, cells * 8}, {o.exp[2], d_jt, 4 * cells * 8}, {occ, d_occ, pairs * 8},
                               {windows, d_win, (size_t)n_rec * 8}});
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_expect_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                               const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off,
                               const int64_t *d_rec_len, int64_t n_rec, double *d_exp_struct, double *d_exp_seq, double *d_occ,
                               int64_t *d_windows)
{
    return expect_profile_dev_any(ctx, "pfmscan_expect_profile_dev", false, struct_tables, seq_tables, n_motifs, m, mode, d_codes, d_profile,
                                  profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec, d_exp_struct, d_exp_seq, nullptr, d_occ, d_windows);
}

int pfmscan_expect_profile_joint_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                     const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off,
                                     const int64_t *d_rec_len, int64_t n_rec, double *d_exp_struct, double *d_exp_seq, double *d_exp_joint,
                                     double *d_occ, int64_t *d_windows)
{
    return expect_profile_dev_any(ctx, "pfmscan_expect_profile_joint_dev", true, struct_tables, seq_tables, n_motifs, m, mode, d_codes, d_profile,
                                  profile_dtype, n_pos, d_rec_off, d_rec_len, n_rec, d_exp_struct, d_exp_seq, d_exp_joint, d_occ, d_windows);
}

int pfmscan_expect_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                  const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_struct, double *exp_seq,
                                  double *occ, int64_t *windows)
{
    const ExppOut o{{exp_struct, exp_seq, nullptr}, {}, {}, false, false};
    return expect_profile_staged_any(ctx, "pfmscan_expect_profile_staged", struct_tables, seq_tables, n_motifs, m, mode, rec_off, rec_len, n_rec, o, occ,
                                     windows);
}

int pfmscan_expect_profile_joint_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                        const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_struct, double *exp_seq,
                                        double *exp_joint, double *occ, int64_t *windows)
{
    const ExppOut o{{exp_struct, exp_seq, exp_joint}, {}, {}, false, true};
    return expect_profile_staged_any(ctx, "pfmscan_expect_profile_joint_staged", struct_tables, seq_tables, n_motifs, m, mode, rec_off, rec_len, n_rec, o,
                                     occ, windows);
}

int pfmscan_expect_profile_merged_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                         const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, uint64_t *acc_struct, uint64_t *acc_seq,
                                         int64_t *bad_struct, int64_t *bad_seq, double *occ, int64_t *windows)
{
    const ExppOut o{{}, {acc_struct, acc_seq, nullptr}, {bad_struct, bad_seq, nullptr}, true, false};
    return expect_profile_staged_any(ctx, "pfmscan_expect_profile_merged_staged", struct_tables, seq_tables, n_motifs, m, mode, rec_off, rec_len,
                                     n_rec, o, occ, windows);
}

int pfmscan_expect_profile_joint_merged_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                               int mode, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, uint64_t *acc_struct,
                                               uint64_t *acc_seq, uint64_t *acc_joint, int64_t *bad_struct, int64_t *bad_seq,
                                               int64_t *bad_joint, double *occ, int64_t *windows)
{
    const ExppOut o{{}, {acc_struct, acc_seq, acc_joint}, {bad_struct, bad_seq, bad_joint}, true, true};
    return expect_profile_staged_any(ctx, "pfmscan_expect_profile_joint_merged_staged", struct_tables, seq_tables, n_motifs, m, mode, rec_off,
                                     rec_len, n_rec, o, occ, windows);
}

}  // extern "C"
