// pfmscan_expect.hip -- expected letter counts per motif column: the E-step of motif refinement (DESIGN.md 5h,
// include/pfmscan.h "expected counts").
//
// The term t_s of window s and whether it has one are the occupancy's (pfmscan_occupancy.hip): the sequential fp64 product
// of the ratio table's cells under the window, none for a window that holds a foreign code.  The weight of a window is its
// term (PFMSCAN_EXPECT_RATIO) or t_s * v with v = 1.0 / occ_r, one rounded division per record and motif and one rounded
// product per window (PFMSCAN_EXPECT_POSTERIOR; occ_r == +0.0: every weight +0.0).  Cell E_r[k][c] is the sum over the
// record's windows of (window has a term and codes[s + k] & 7 == c) ? w_s : +0.0 in the occupancy's left-aligned tree of
// fan-in 32 anchored at the record's first window.  No transcendental, no atomics, no tolerance: tests/expect_rules.py
// restates it in numpy and the bits are compared.
//
//   k_exp_inverse   v of every (record, motif) from the occupancy, which the call computes first over the same records
//                   (occ_run); -1.0 stands for "occ_r is +0.0" (no other v is negative).
//   k_exp_group_records  before it, per range of records: the record of every workgroup's first block.
//   k_exp_blocks    level 0.  A workgroup owns 8 consecutive blocks of the pass, 32 lanes each: a lane per window.  The
//                   block's 32 + m - 1 codes are parked in LDS (foreign ones as 0xFF); for every motif of the pass a lane
//                   makes its window's term from the motif's table in LDS and parks the weight (+0.0 for a window without a
//                   term or beyond the record) in LDS; then a lane per (block, column k, letter c) walks the block's 32
//                   weights in order and adds (code[w + k] == c ? weight : +0.0) from 0.0.  One writer per scratch cell.
//                   Nothing is indexed at run time but LDS.
//   k_exp_pair_blocks   level 0 on two code streams: the same plan with both strips of a block in LDS, the joint
//                   weight made once per pair and the 4 + 7 columns of a matrix row (pair, k) summed together; described
//                   above the kernel.
// The m x n_letters cells of a motif are independent columns of block sums: levels 1 and up are the occupancy's own
// k_occ_level1 and k_occ_finish (occ_launch_upper), which store column row * n_letters + c at [row][c] of the [m][8] matrix.
// Scratch is blocks x columns doubles under the occupancy's cap: records run in passes, and when the longest record alone
// passes the cap, so do the columns (cells, then motifs): occ_plan (pfmscan_occ_plan.hpp) over columns, or over the matrix rows
// of pairs.  The two level-0 kernels share how a lane finds its block and what it parks in a strip (exp_block, exp_code).
#include <algorithm>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_occ.hpp"

#pragma clang fp contract(off)   // products and sums are rounded one operation at a time: never an FMA

namespace pfmscan {

constexpr int EXP_WB = BLOCK / OCC_FANIN;                          // blocks of a workgroup
constexpr int EXP_CS = (OCC_FANIN + PFMSCAN_MAX_M - 1 + 3) / 4 * 4;   // bytes of a block's strip of codes
constexpr uint8_t EXP_FOREIGN = 0xFF;
static_assert(EXP_WB * OCC_FANIN == BLOCK && EXP_CS >= OCC_FANIN + PFMSCAN_MAX_M - 1, "a lane per window");

__global__ __launch_bounds__(BLOCK) void k_exp_inverse(const double *__restrict__ occ, double *__restrict__ inv, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double o = occ[i];
    inv[i] = o == 0.0 ? -1.0 : 1.0 / o;
}

int exp_launch_inverse(pfmscan_ctx *ctx, const double *d_occ, double *d_inv, int64_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_exp_inverse, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_occ, d_inv, n);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail_hip(ctx, e, "k_exp_inverse") : PFMSCAN_OK;
}

// the record of the first block of every workgroup of k_exp_blocks, so that a workgroup finds its records with two round trips
// to memory and a short walk instead of a bisection of ~17 dependent loads (as k_occ_run_records does for the profile kernel)
__global__ __launch_bounds__(BLOCK) void k_exp_group_records(const OccArgs a, int64_t *__restrict__ wg_rec)
{
    const int64_t r = a.r0 + (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= a.r1) return;
    const int64_t b0 = a.blk_start[r] - a.blk_base, b1 = a.blk_start[r + 1] - a.blk_base;   // a record without a block claims nothing
    for (int64_t u = (b0 + EXP_WB - 1) / EXP_WB; u * EXP_WB < b1; ++u) wg_rec[u] = r;
}

// ---- what the two level-0 kernels share: a workgroup owns EXP_WB consecutive blocks of the pass, 32 lanes each ---------------
struct ExpBlock {
    int64_t r;                   // the block's record
    int64_t s0;                  // its first position in the stream
    int nw;                      // its windows, >= 1
    int need;                    // its codes, nw + m - 1: all inside the record
};

// block gb < a.n_blk of the pass: its record by a short walk from the record of the workgroup's first block (wg_rec, written by
// k_exp_group_records), and its geometry
__device__ __forceinline__ ExpBlock exp_block(const OccArgs &a, const int64_t *__restrict__ wg_rec, int64_t gb)
{
    const int64_t b = a.blk_base + gb;
    int64_t r = wg_rec[blockIdx.x];
    while (a.blk_start[r + 1] <= b) ++r;                           // ends inside the pass: blk_start[r1] > b
    const int64_t w0 = (b - a.blk_start[r]) * OCC_FANIN;
    const int nw = (int)min((int64_t)OCC_FANIN, a.rec_len[r] - a.m + 1 - w0);   // >= 1: the block exists
    return ExpBlock{r, a.rec_off[r] + w0, nw, nw + a.m - 1};
}

// the strip's byte for code i of the block: codes >= nl and what lies beyond the block as EXP_FOREIGN
__device__ __forceinline__ uint8_t exp_code(const uint8_t *codes, const ExpBlock &blk, int i, int nl)
{
    if (i >= blk.need) return EXP_FOREIGN;
    const uint8_t x = codes[blk.s0 + i] & 7u;
    return (int)x < nl ? x : EXP_FOREIGN;
}

// a.q_first / a.n_q: the columns of the pass, column = (motif * m + k) * n_letters + c; inv [n_rec][n_motifs] or null (ratio mode)
__global__ __launch_bounds__(BLOCK) void k_exp_blocks(const OccArgs a, const double *__restrict__ inv, const int64_t *__restrict__ wg_rec)
{
    __shared__ double tab[PFMSCAN_MAX_M * 8];
    __shared__ double wl[EXP_WB][OCC_FANIN + 1];
    __shared__ uint8_t cl[EXP_WB][EXP_CS];
    const int t = threadIdx.x, j = t >> 5, w = t & 31, m = a.m, nl = a.n_letters;
    const int64_t gb = (int64_t)blockIdx.x * EXP_WB + j;           // this lane's block, within the pass
    const bool live = gb < a.n_blk;
    ExpBlock blk{};
    if (live) {
        blk = exp_block(a, wg_rec, gb);
        for (int i = w; i < EXP_CS; i += OCC_FANIN) cl[j][i] = exp_code(a.codes, blk, i, nl);
    }
    __syncthreads();
    bool has = live && w < blk.nw;                                 // this lane's window has a term
    if (has)
        for (int k = 0; k < m; ++k) has = has && cl[j][w + k] != EXP_FOREIGN;
    const int64_t r = blk.r;
    const int mc = m * nl;                                         // cells of a motif
    const int c_lo = a.q_first, c_hi = a.q_first + a.n_q;
    const int q_lo = c_lo / mc;
    for (int q = q_lo; q * mc < c_hi; ++q) {
        if (q != q_lo) __syncthreads();                            // the adders of the last motif are done with wl
        for (int i = t; i < m * 8; i += BLOCK) tab[i] = a.tables[(int64_t)q * m * 8 + i];
        __syncthreads();
        double wt = 0.0;
        if (has) {
            const uint8_t *cp = &cl[j][w];
            double x = tab[cp[0]];
            for (int k = 1; k < m; ++k) x = x * tab[k * 8 + cp[k]];
            if (inv) {
                const double v = inv[r * a.n_motifs + q];
                x = v < 0.0 ? 0.0 : x * v;
            }
            wt = x;
        }
        wl[j][w] = wt;
        __syncthreads();
        if (live) {
            const int lo = max(c_lo - q * mc, 0), hi = min(c_hi - q * mc, mc);   // the motif's cells that are columns of the pass
            double *out = a.bs + gb * a.n_q + (q * mc - c_lo);
            for (int cc = lo + w; cc < hi; cc += OCC_FANIN) {
                const int k = nl == 4 ? cc >> 2 : cc / PFMSCAN_NSTRUCT, c = cc - k * nl;
                const uint8_t *cp = &cl[j][k];
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < OCC_FANIN; ++i) s = s + ((int)cp[i] == c ? wl[j][i] : 0.0);
                out[cc] = s;
            }
        }
    }
}

// ---- two code streams (include/pfmscan.h "occupancy and expected counts of two code streams") -----------------
// k_exp_blocks with a second stream.  Both strips of a block are parked in LDS (foreign codes as 0xFF, each in its own
// stream); a window has a term when no position under it is foreign in either.  Per pair a lane makes its window's term by
// the joint chain (the letters over R, then the structure letters over S: 2 m - 1 rounded products) and its weight ONCE and
// parks it; then a lane per (block, k, letter) of the 4 + 7 columns of the matrix rows (pair, k) of the pass walks the
// block's 32 weights in order and adds (code == letter ? weight : +0.0) from 0.0 -- letters 0..3 against the RNA strip into
// bs_seq, 4..10 against the structure strip into bs_struct.  A region that is null is not computed.  One writer per cell.
// JOINT: the 4 x 7 table of a matrix row as well (bs_joint, never null then).  A third strip holds a | b << 3 per position
// (0xFF where either code is foreign: the packing of k_occ_blocks<QN, true>), and a lane per (block, k, a, b) walks the same 32
// weights against it: one compare per step.  A weight that is not +0.0 belongs to a window without a foreign position, so the
// packed byte under it is that of two known letters.  Without JOINT nothing of this is compiled.
struct ExpPairArgs {
    const double *inv;           // [n_rec][n_motifs] or null (ratio mode)
    double *bs_seq;              // [n_blk][n_u * 4] or null
    double *bs_struct;           // [n_blk][n_u * 7] or null
    double *bs_joint;            // [n_blk][n_u * 28]: column (u * 4 + a) * 7 + b; null without JOINT
    int u_first, n_u;            // matrix rows of the pass: u = pair * m + k
};
constexpr int EXP_NJ = 4 * PFMSCAN_NSTRUCT;                        // cells of the joint table of a matrix row
constexpr int EXP_FILL_ROUNDS = 16;                                // workgroups per CU a pass with the table should have (5 are resident)

template <bool JOINT>
__global__ __launch_bounds__(BLOCK) void k_exp_pair_blocks(const OccArgs a, const ExpPairArgs e, const int64_t *__restrict__ wg_rec)
{
    __shared__ double tab[2][PFMSCAN_MAX_M * 8];
    __shared__ double wl[EXP_WB][OCC_FANIN + 1];
    __shared__ uint8_t cl[2][EXP_WB][EXP_CS];
    __shared__ uint8_t pl[JOINT ? EXP_WB : 1][EXP_CS];
    constexpr int NS = PFMSCAN_NSTRUCT, NC = 4 + NS;
    const int t = threadIdx.x, j = t >> 5, w = t & 31, m = a.m;
    const int64_t gb = (int64_t)blockIdx.x * EXP_WB + j;           // this lane's block, within the pass
    const bool live = gb < a.n_blk;
    ExpBlock blk{};
    if (live) {
        blk = exp_block(a, wg_rec, gb);
        for (int i = w; i < EXP_CS; i += OCC_FANIN) {              // both strips in one walk (a walk per strip measured 3 % slower)
            const uint8_t x = exp_code(a.codes, blk, i, 4), y = exp_code(a.codes2, blk, i, NS);
            cl[0][j][i] = x;
            cl[1][j][i] = y;
            if constexpr (JOINT) pl[j][i] = x == EXP_FOREIGN || y == EXP_FOREIGN ? EXP_FOREIGN : (uint8_t)(x | (y << 3));
        }
    }
    __syncthreads();
    bool has = live && w < blk.nw;                                 // this lane's window has a term
    if (has)
        for (int k = 0; k < m; ++k) has = has && cl[0][j][w + k] != EXP_FOREIGN && cl[1][j][w + k] != EXP_FOREIGN;
    const int64_t r = blk.r;
    const int u_lo = e.u_first, u_hi = e.u_first + e.n_u;
    const int q_lo = u_lo / m;
    const int64_t sq = (int64_t)e.n_u * 4, ss = (int64_t)e.n_u * NS;   // doubles per block of the two scratch regions
    for (int q = q_lo; q * m < u_hi; ++q) {
        if (q != q_lo) __syncthreads();                            // the adders of the last pair are done with wl
        for (int i = t; i < m * 8; i += BLOCK) {
            tab[0][i] = a.tables[(int64_t)q * m * 8 + i];
            tab[1][i] = a.tables2[(int64_t)q * m * 8 + i];
        }
        __syncthreads();
        double wt = 0.0;
        if (has) {
            const uint8_t *cp = &cl[0][j][w];
            double x = tab[0][cp[0]];
            for (int k = 1; k < m; ++k) x = x * tab[0][k * 8 + cp[k]];
            cp = &cl[1][j][w];
            for (int k = 0; k < m; ++k) x = x * tab[1][k * 8 + cp[k]];
            if (e.inv) {
                const double v = e.inv[r * a.n_motifs + q];
                x = v < 0.0 ? 0.0 : x * v;
            }
            wt = x;
        }
        wl[j][w] = wt;
        __syncthreads();
        if (live) {
            const int k_lo = max(u_lo - q * m, 0), k_hi = min(u_hi - q * m, m);   // the pair's matrix rows that are rows of the pass
            const int items = (k_hi - k_lo) * NC;
            for (int it = w; it < items; it += OCC_FANIN) {
                const int kk = it / NC, c = it - kk * NC, k = k_lo + kk;
                const bool st = c >= 4;
                double *region = st ? e.bs_struct : e.bs_seq;
                if (!region) continue;
                const int letter = st ? c - 4 : c;
                const uint8_t *cp = &cl[st ? 1 : 0][j][k];
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < OCC_FANIN; ++i) s = s + ((int)cp[i] == letter ? wl[j][i] : 0.0);
                const int64_t u = (int64_t)q * m + k - u_lo;
                if (st) region[gb * ss + u * NS + letter] = s;
                else region[gb * sq + u * 4 + letter] = s;
            }
            if constexpr (JOINT) {
                double *out = e.bs_joint + gb * ((int64_t)e.n_u * EXP_NJ) + ((int64_t)q * m + k_lo - u_lo) * EXP_NJ;
                for (int it = w; it < (k_hi - k_lo) * EXP_NJ; it += OCC_FANIN) {   // it = kk * 28 + a * 7 + b: the column within the pair's rows
                    const int kk = it / EXP_NJ, c = it - kk * EXP_NJ, ca = c / NS;
                    const int want = ca | ((c - ca * NS) << 3);
                    const uint8_t *cp = &pl[j][k_lo + kk];
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < OCC_FANIN; ++i) s = s + ((int)cp[i] == want ? wl[j][i] : 0.0);
                    out[it] = s;
                }
            }
        }
    }
}

// room for a pass's workgroup -> record table, in ctx->occ_cnt
static int exp_wg_rec(pfmscan_ctx *ctx, const OccPlan &p, int64_t *&wg_rec)
{
    const int rc = ensure(ctx, ctx->occ_cnt, std::max<size_t>((size_t)((p.need_blk + EXP_WB - 1) / EXP_WB) * 8, 16));
    wg_rec = (int64_t *)ctx->occ_cnt.p;
    return rc;
}

// Launches on st, does not wait.  d_exp_seq / d_exp_struct / d_exp_joint: at least one is not null.
static int exp_pair_run(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                        const uint8_t *d_codes, const uint8_t *d_codes2, const OccRecords &rec, double *d_exp_seq, double *d_exp_struct,
                        double *d_exp_joint, double *d_occ, int64_t *d_windows, hipStream_t st)
{
    int rc;
    const bool posterior = mode == PFMSCAN_EXPECT_POSTERIOR;
    const int64_t pairs = rec.n_rec * n_motifs;
    const int64_t n_unit = (int64_t)n_motifs * m;                  // matrix rows (pair, k)
    const int wide = d_exp_joint ? EXP_NJ : PFMSCAN_NSTRUCT;       // columns of a matrix row in the widest matrix of the call
    if (n_unit * wide > (int64_t(1) << 30)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many motifs for one call");
    // the occupancy of the same records first: v of posterior mode, and what the caller asked for
    if (posterior || d_occ || d_windows) {
        if (!d_occ) {
            if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
            d_occ = (double *)ctx->exp_occ.p;
        }
        const OccPair pr{struct_tables, d_codes2};
        if ((rc = occ_run(ctx, who, seq_tables, n_motifs, m, 4, d_codes, rec, d_occ, d_windows, st, nullptr, &pr))) return rc;
    }
    ExpPairArgs e{};
    if (posterior) {
        if ((rc = ensure(ctx, ctx->exp_inv, (size_t)pairs * 8))) return rc;
        if ((rc = exp_launch_inverse(ctx, d_occ, (double *)ctx->exp_inv.p, pairs, st))) return rc;
        e.inv = (const double *)ctx->exp_inv.p;
    }
    // the columns past the letters of every matrix row are +0.0; every other cell is written by k_occ_finish
    if (d_exp_seq) HIP_TRY(ctx, hipMemsetAsync(d_exp_seq, 0, (size_t)pairs * m * 8 * sizeof(double), st));
    if (d_exp_struct) HIP_TRY(ctx, hipMemsetAsync(d_exp_struct, 0, (size_t)pairs * m * 8 * sizeof(double), st));
    if (d_exp_joint) HIP_TRY(ctx, hipMemsetAsync(d_exp_joint, 0, (size_t)pairs * m * 4 * 8 * sizeof(double), st));
    // matrix rows per pass: all of them unless the longest record's block sums alone pass the cap; then records per pass
    const int nsq = d_exp_seq ? 4 : 0, nst = d_exp_struct ? PFMSCAN_NSTRUCT : 0;
    const int cells = nsq + nst + (d_exp_joint ? EXP_NJ : 0);      // scratch doubles of a matrix row, all regions
    // with the table a matrix row takes 39 doubles of a block, and all rows of a library in a pass would leave room for a few
    // records only: a pass then holds whole pairs, as many as leave room for the blocks of a few rounds of workgroups
    const int64_t fill_blk = d_exp_joint ? (int64_t)EXP_FILL_ROUNDS * std::max(ctx->n_cu, 1) * EXP_WB : 1;
    const OccPlan p = occ_plan(rec.len, rec.n_rec, m, n_unit, cells, wide, occ_scratch_cap(), false, fill_blk, d_exp_joint ? m : 1);
    if ((p.need_blk + EXP_WB - 1) / EXP_WB > 0x7FFFFFFF) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": a record is too long for one call");
    OccArgs a{};
    if ((rc = occ_upload_tables(ctx, seq_tables, struct_tables, (size_t)n_motifs * m * 8 * sizeof(double), n_motifs, m, st, a.tables, a.tables2))) return rc;
    if ((rc = occ_frame(ctx, p, cells, rec, n_motifs, m, 4, st, a))) return rc;
    int64_t *wg_rec;
    if ((rc = exp_wg_rec(ctx, p, wg_rec))) return rc;
    a.codes = d_codes;
    a.codes2 = d_codes2;
    a.out_stride = (int64_t)n_motifs * m * 8;
    // the scratch regions of a pass: the sequence matrix's block and level-1 sums, then the structure matrix's, then the table's
    double *bs_struct = a.bs + p.need_blk * p.n_u_max * nsq, *gs_struct = a.gs + p.need_grp * p.n_u_max * nsq;
    e.bs_seq = d_exp_seq ? a.bs : nullptr;
    e.bs_struct = d_exp_struct ? bs_struct : nullptr;
    e.bs_joint = d_exp_joint ? bs_struct + p.need_blk * p.n_u_max * nst : nullptr;
    OccArgs as = a;                                                // levels 1 and up of the structure matrix
    OccArgs aj = a;                                                // and of the table: a matrix of 4 m rows (k, a) and 7 letters
    aj.bs = e.bs_joint;
    aj.gs = gs_struct + p.need_grp * p.n_u_max * nst;
    aj.occ = d_exp_joint;
    aj.out_stride = a.out_stride * 4;
    aj.cell_nl = PFMSCAN_NSTRUCT;
    a.occ = d_exp_seq;
    a.cell_nl = 4;
    as.bs = bs_struct;
    as.gs = gs_struct;
    as.occ = d_exp_struct;
    as.cell_nl = PFMSCAN_NSTRUCT;
    for (int64_t u0 = 0; u0 < n_unit; u0 += p.n_u_max) {
        e.u_first = (int)u0;
        e.n_u = (int)std::min<int64_t>(p.n_u_max, n_unit - u0);
        a.q_first = e.u_first * 4;
        a.n_q = e.n_u * 4;
        as.q_first = e.u_first * PFMSCAN_NSTRUCT;
        as.n_q = e.n_u * PFMSCAN_NSTRUCT;
        aj.q_first = e.u_first * EXP_NJ;
        aj.n_q = e.n_u * EXP_NJ;
        for (size_t i = 0; i < p.n_pass(); ++i) {
            const bool make_table = p.n_pass() > 1 || u0 == 0;     // one range of records: its table is made once, for all passes over the rows
            occ_set_pass(a, p, i);
            occ_set_pass(as, p, i);
            occ_set_pass(aj, p, i);
            if (a.n_blk > 0) {
                if (make_table) hipLaunchKernelGGL(k_exp_group_records, dim3((unsigned)((a.r1 - a.r0 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, a, wg_rec);
                const dim3 grid((unsigned)((a.n_blk + EXP_WB - 1) / EXP_WB));
                if (d_exp_joint) hipLaunchKernelGGL(k_exp_pair_blocks<true>, grid, dim3(BLOCK), 0, st, a, e, wg_rec);
                else hipLaunchKernelGGL(k_exp_pair_blocks<false>, grid, dim3(BLOCK), 0, st, a, e, wg_rec);
                hipError_t err = hipGetLastError();
                if (err != hipSuccess) return fail_hip(ctx, err, "k_exp_pair_blocks");
            }
            if (d_exp_seq && (rc = occ_launch_upper(ctx, a, st))) return rc;
            if (d_exp_struct && (rc = occ_launch_upper(ctx, as, st))) return rc;
            if (d_exp_joint && (rc = occ_launch_upper(ctx, aj, st))) return rc;
        }
    }
    return PFMSCAN_OK;
}

// Launches on st, does not wait.
static int exp_run(pfmscan_ctx *ctx, const char *who, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                   const uint8_t *d_codes, const OccRecords &rec, double *d_exp, double *d_occ, int64_t *d_windows, hipStream_t st)
{
    int rc;
    const bool posterior = mode == PFMSCAN_EXPECT_POSTERIOR;
    const int64_t pairs = rec.n_rec * n_motifs;
    const int64_t n_col = (int64_t)n_motifs * m * n_letters;
    if (n_col > (int64_t(1) << 30)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many motifs for one call");
    // the occupancy of the same records first: v of posterior mode, and what the caller asked for
    if (posterior || d_occ || d_windows) {
        if (!d_occ) {
            if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
            d_occ = (double *)ctx->exp_occ.p;
        }
        if ((rc = occ_run(ctx, who, ratio_tables, n_motifs, m, n_letters, d_codes, rec, d_occ, d_windows, st))) return rc;
    }
    const double *d_inv = nullptr;
    if (posterior) {
        if ((rc = ensure(ctx, ctx->exp_inv, (size_t)pairs * 8))) return rc;
        if ((rc = exp_launch_inverse(ctx, d_occ, (double *)ctx->exp_inv.p, pairs, st))) return rc;
        d_inv = (const double *)ctx->exp_inv.p;
    }
    // the columns >= n_letters of every matrix row are +0.0; every other cell is written by k_occ_finish
    HIP_TRY(ctx, hipMemsetAsync(d_exp, 0, (size_t)pairs * m * 8 * sizeof(double), st));
    // columns per pass: all of them unless the longest record's block sums alone pass the cap; then records per pass
    const OccPlan p = occ_plan(rec.len, rec.n_rec, m, n_col, 1, 1, occ_scratch_cap(), false);
    if ((p.need_blk + EXP_WB - 1) / EXP_WB > 0x7FFFFFFF) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": a record is too long for one call");
    OccArgs a{};
    const double *none;
    if ((rc = occ_upload_tables(ctx, ratio_tables, nullptr, 0, n_motifs, m, st, a.tables, none))) return rc;
    if ((rc = occ_frame(ctx, p, 1, rec, n_motifs, m, n_letters, st, a))) return rc;
    int64_t *wg_rec;
    if ((rc = exp_wg_rec(ctx, p, wg_rec))) return rc;
    a.codes = d_codes;
    a.occ = d_exp;
    a.out_stride = (int64_t)n_motifs * m * 8;
    a.cell_nl = n_letters;
    for (int64_t c0 = 0; c0 < n_col; c0 += p.n_u_max) {
        a.q_first = (int)c0;
        a.n_q = (int)std::min<int64_t>(p.n_u_max, n_col - c0);
        for (size_t i = 0; i < p.n_pass(); ++i) {
            const bool make_table = p.n_pass() > 1 || c0 == 0;     // one range of records: its table is made once, for all passes over the columns
            occ_set_pass(a, p, i);
            if (a.n_blk > 0) {
                if (make_table) hipLaunchKernelGGL(k_exp_group_records, dim3((unsigned)((a.r1 - a.r0 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, a, wg_rec);
                hipLaunchKernelGGL(k_exp_blocks, dim3((unsigned)((a.n_blk + EXP_WB - 1) / EXP_WB)), dim3(BLOCK), 0, st, a, d_inv, wg_rec);
                hipError_t e = hipGetLastError();
                if (e != hipSuccess) return fail_hip(ctx, e, "k_exp_blocks");
            }
            if ((rc = occ_launch_upper(ctx, a, st))) return rc;
        }
    }
    return PFMSCAN_OK;
}

static int exp_check_mode(pfmscan_ctx *ctx, const char *who, int mode)
{
    if (mode != PFMSCAN_EXPECT_RATIO && mode != PFMSCAN_EXPECT_POSTERIOR)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": mode must be PFMSCAN_EXPECT_RATIO or PFMSCAN_EXPECT_POSTERIOR");
    return PFMSCAN_OK;
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_expect_dev(pfmscan_ctx *ctx, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                       const uint8_t *d_codes, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec,
                       double *d_exp, double *d_occ, int64_t *d_windows)
{
    const char *who = "pfmscan_expect_dev";
    if (int rc = occ_check(ctx, who, ratio_tables, n_motifs, m, n_letters, n_pos, n_rec)) return rc;
    if (int rc = exp_check_mode(ctx, who, mode)) return rc;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || !d_exp || (n_pos > 0 && !d_codes)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table, codes or output");
    if (misaligned(d_codes)) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    return exp_run(ctx, who, ratio_tables, n_motifs, m, n_letters, mode, d_codes, rec, d_exp, d_occ, d_windows, ctx->stream);
}

// both _staged forms: the matrices come home (exp), or their exact sums over the records do (acc, bad: the merged form)
static int expect_staged_any(pfmscan_ctx *ctx, const char *who, int which, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp, uint64_t *acc, int64_t *bad, bool merged,
                             double *occ, int64_t *windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (which != 0 && which != 1) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": which must be 0 (codes) or 1 (codes2)");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && !(which ? ctx->staged_codes2 : ctx->staged_codes))
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + (which ? ": no codes2 are staged (pfmscan_stage_codes2)" : ": no codes are staged"));
    if (int rc = occ_check(ctx, who, ratio_tables, n_motifs, m, n_letters, ctx->staged_n, n_rec)) return rc;
    if (int rc = exp_check_mode(ctx, who, mode)) return rc;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len || (merged ? !acc || !bad : !exp)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or output");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const size_t pairs = (size_t)n_rec * n_motifs, cells = pairs * m * 8;
    if ((rc = ensure(ctx, ctx->exp_out, (cells + pairs + (size_t)n_rec) * 8))) return rc;
    double *d_exp = (double *)ctx->exp_out.p;
    double *d_occ = occ ? d_exp + cells : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_exp + cells + pairs) : nullptr;
    const uint8_t *d_codes = (const uint8_t *)(which ? ctx->codes2.p : ctx->codes.p);
    if ((rc = exp_run(ctx, who, ratio_tables, n_motifs, m, n_letters, mode, d_codes, rec, d_exp, d_occ, d_win, ctx->stream))) return rc;
    if (merged) {
        const ExpMergeOut out{d_exp, acc, bad, m};
        return exp_merge_home(ctx, who, &out, 1, n_rec, n_motifs, m, d_occ, occ, d_win, windows);
    }
    return occ_copy_home(ctx, {{exp, d_exp, cells * 8}, {occ, d_occ, pairs * 8}, {windows, d_win, (size_t)n_rec * 8}});
}

int pfmscan_expect_staged(pfmscan_ctx *ctx, int which, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                          const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp, double *occ, int64_t *windows)
{
    return expect_staged_any(ctx, "pfmscan_expect_staged", which, ratio_tables, n_motifs, m, n_letters, mode, rec_off, rec_len, n_rec, exp, nullptr,
                             nullptr, false, occ, windows);
}

int pfmscan_expect_merged_staged(pfmscan_ctx *ctx, int which, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                                 const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, uint64_t *acc, int64_t *bad, double *occ,
                                 int64_t *windows)
{
    return expect_staged_any(ctx, "pfmscan_expect_merged_staged", which, ratio_tables, n_motifs, m, n_letters, mode, rec_off, rec_len, n_rec, nullptr,
                             acc, bad, true, occ, windows);
}

// the _dev form of two code streams.  table: the form has a d_exp_joint (null there: the table is not asked for)
static int expect_pair_dev_any(pfmscan_ctx *ctx, const char *who, bool table, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                               int mode, const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                               const int64_t *d_rec_len, int64_t n_rec, double *d_exp_seq, double *d_exp_struct, double *d_exp_joint, double *d_occ,
                               int64_t *d_windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = occ_pair_check(ctx, who, seq_tables, struct_tables, n_motifs, m, n_pos, n_rec)) return rc;
    if (int rc = exp_check_mode(ctx, who, mode)) return rc;
    if (!d_exp_seq && !d_exp_struct && !d_exp_joint)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + (table ? ": d_exp_seq, d_exp_struct and d_exp_joint are all NULL" : ": d_exp_seq and d_exp_struct are both NULL"));
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || (n_pos > 0 && (!d_codes || !d_codes2))) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or codes");
    if (misaligned(d_codes) || misaligned(d_codes2)) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    return exp_pair_run(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, d_codes, d_codes2, rec, d_exp_seq, d_exp_struct, d_exp_joint, d_occ,
                        d_windows, ctx->stream);
}

int pfmscan_expect_pair_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                            const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                            const int64_t *d_rec_len, int64_t n_rec, double *d_exp_seq, double *d_exp_struct, double *d_occ,
                            int64_t *d_windows)
{
    return expect_pair_dev_any(ctx, "pfmscan_expect_pair_dev", false, seq_tables, struct_tables, n_motifs, m, mode, d_codes, d_codes2, n_pos, d_rec_off,
                               d_rec_len, n_rec, d_exp_seq, d_exp_struct, nullptr, d_occ, d_windows);
}

int pfmscan_expect_pair_joint_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                                  const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                                  const int64_t *d_rec_len, int64_t n_rec, double *d_exp_seq, double *d_exp_struct, double *d_exp_joint,
                                  double *d_occ, int64_t *d_windows)
{
    return expect_pair_dev_any(ctx, "pfmscan_expect_pair_joint_dev", true, seq_tables, struct_tables, n_motifs, m, mode, d_codes, d_codes2, n_pos,
                               d_rec_off, d_rec_len, n_rec, d_exp_seq, d_exp_struct, d_exp_joint, d_occ, d_windows);
}

// the outputs of a _staged form of two code streams: the matrices on the HOST (exp), or with merged their accumulators and
// verdicts; [0] sequence, [1] structure, [2] the table (table: the form has one; null there: not asked for)
struct ExpPairOut {
    double *exp[3];
    uint64_t *acc[3];
    int64_t *bad[3];
    bool merged, table;
};

// both _staged forms of two code streams
static int expect_pair_staged_any(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                                  const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const ExpPairOut &o, double *occ, int64_t *windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes are staged");
    if (ctx->staged_n > 0 && !ctx->staged_codes2) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes2 are staged (pfmscan_stage_codes2)");
    if (int rc = occ_pair_check(ctx, who, seq_tables, struct_tables, n_motifs, m, ctx->staged_n, n_rec)) return rc;
    if (int rc = exp_check_mode(ctx, who, mode)) return rc;
    bool want[3];
    for (int i = 0; i < 3; ++i) want[i] = o.merged ? o.acc[i] != nullptr : o.exp[i] != nullptr;
    if (!want[0] && !want[1] && !want[2]) {
        const char *none = o.table ? (o.merged ? ": acc_seq, acc_struct and acc_joint are all NULL" : ": exp_seq, exp_struct and exp_joint are all NULL")
                                   : (o.merged ? ": acc_seq and acc_struct are both NULL" : ": exp_seq and exp_struct are both NULL");
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + none);
    }
    for (int i = 0; i < 3; ++i)
        if (o.merged && want[i] && !o.bad[i]) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": an accumulator without its bad");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const size_t pairs = (size_t)n_rec * n_motifs, cells = pairs * m * 8, all = (want[2] ? 6 : 2) * cells;   // the table is four matrices wide
    if ((rc = ensure(ctx, ctx->exp_out, (all + pairs + (size_t)n_rec) * 8))) return rc;
    double *d_base = (double *)ctx->exp_out.p;
    double *d_sq = want[0] ? d_base : nullptr;
    double *d_st = want[1] ? d_base + cells : nullptr;
    double *d_jt = want[2] ? d_base + 2 * cells : nullptr;
    double *d_occ = occ ? d_base + all : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_base + all + pairs) : nullptr;
    if ((rc = exp_pair_run(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, (const uint8_t *)ctx->codes.p, (const uint8_t *)ctx->codes2.p, rec,
                           d_sq, d_st, d_jt, d_occ, d_win, ctx->stream)))
        return rc;
    if (o.merged) {
        const ExpMergeOut out[3] = {{d_sq, o.acc[0], o.bad[0], m}, {d_st, o.acc[1], o.bad[1], m}, {d_jt, o.acc[2], o.bad[2], 4 * m}};
        return exp_merge_home(ctx, who, out, 3, n_rec, n_motifs, m, d_occ, occ, d_win, windows);
    }
    return occ_copy_home(ctx, {{o.exp[0], d_sq, cells * 8}, {o.exp[1], d_st, cells * 8}, {o.exp[2], d_jt, 4 * cells * 8}, {occ, d_occ, pairs * 8},
                               {windows, d_win, (size_t)n_rec * 8}});
}

int pfmscan_expect_pair_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                               const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_seq, double *exp_struct,
                               double *occ, int64_t *windows)
{
    const ExpPairOut o{{exp_seq, exp_struct, nullptr}, {}, {}, false, false};
    return expect_pair_staged_any(ctx, "pfmscan_expect_pair_staged", seq_tables, struct_tables, n_motifs, m, mode, rec_off, rec_len, n_rec, o, occ, windows);
}

int pfmscan_expect_pair_joint_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                                     const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp_seq, double *exp_struct,
                                     double *exp_joint, double *occ, int64_t *windows)
{
    const ExpPairOut o{{exp_seq, exp_struct, exp_joint}, {}, {}, false, true};
    return expect_pair_staged_any(ctx, "pfmscan_expect_pair_joint_staged", seq_tables, struct_tables, n_motifs, m, mode, rec_off, rec_len, n_rec, o, occ,
                                  windows);
}

int pfmscan_expect_pair_merged_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                                      const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, uint64_t *acc_seq, uint64_t *acc_struct,
                                      int64_t *bad_seq, int64_t *bad_struct, double *occ, int64_t *windows)
{
    const ExpPairOut o{{}, {acc_seq, acc_struct, nullptr}, {bad_seq, bad_struct, nullptr}, true, false};
    return expect_pair_staged_any(ctx, "pfmscan_expect_pair_merged_staged", seq_tables, struct_tables, n_motifs, m, mode, rec_off, rec_len, n_rec, o, occ,
                                  windows);
}

int pfmscan_expect_pair_joint_merged_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                                            const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, uint64_t *acc_seq, uint64_t *acc_struct,
                                            uint64_t *acc_joint, int64_t *bad_seq, int64_t *bad_struct, int64_t *bad_joint, double *occ,
                                            int64_t *windows)
{
    const ExpPairOut o{{}, {acc_seq, acc_struct, acc_joint}, {bad_seq, bad_struct, bad_joint}, true, true};
    return expect_pair_staged_any(ctx, "pfmscan_expect_pair_joint_merged_staged", seq_tables, struct_tables, n_motifs, m, mode, rec_off, rec_len, n_rec, o,
                                  occ, windows);
}

}  // extern "C"
