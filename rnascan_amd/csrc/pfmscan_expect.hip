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
//                   (occ_run_letters); -1.0 stands for "occ_r is +0.0" (no other v is negative).
//   k_exp_group_records  before it, per range of records: the record of every workgroup's first block.
//   k_exp_blocks    level 0.  A workgroup owns 8 consecutive blocks of the pass, 32 lanes each: a lane per window.  The
//                   block's 32 + m - 1 codes are parked in LDS (foreign ones as 0xFF); for every motif of the pass a lane
//                   makes its window's term from the motif's table in LDS and parks the weight (+0.0 for a window without a
//                   term or beyond the record) in LDS; then a lane per (block, column k, letter c) walks the block's 32
//                   weights in order and adds (code[w + k] == c ? weight : +0.0) from 0.0.  One writer per scratch cell.
//                   Nothing is indexed at run time but LDS.
// The m x n_letters cells of a motif are independent columns of block sums: levels 1 and up are the occupancy's own
// k_occ_level1 and k_occ_finish (occ_launch_upper), which store column row * n_letters + c at [row][c] of the [m][8] matrix.
// Scratch is blocks x columns doubles under the occupancy's cap: records run in passes, and when the longest record alone
// passes the cap, so do the columns (cells, then motifs).
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

// a.q_first / a.n_q: the columns of the pass, column = (motif * m + k) * n_letters + c; inv [n_rec][n_motifs] or null (ratio mode)
__global__ __launch_bounds__(BLOCK) void k_exp_blocks(const OccArgs a, const double *__restrict__ inv, const int64_t *__restrict__ wg_rec)
{
    __shared__ double tab[PFMSCAN_MAX_M * 8];
    __shared__ double wl[EXP_WB][OCC_FANIN + 1];
    __shared__ uint8_t cl[EXP_WB][EXP_CS];
    const int t = threadIdx.x, j = t >> 5, w = t & 31, m = a.m, nl = a.n_letters;
    const int64_t gb = (int64_t)blockIdx.x * EXP_WB + j;           // this lane's block, within the pass
    const bool live = gb < a.n_blk;
    int64_t r = 0;
    int nw = 0;
    if (live) {
        const int64_t b = a.blk_base + gb;
        r = wg_rec[blockIdx.x];                                    // the record of the workgroup's first block
        while (a.blk_start[r + 1] <= b) ++r;                       // ends inside the pass: blk_start[r1] > b
        const int64_t w0 = (b - a.blk_start[r]) * OCC_FANIN;
        nw = (int)min((int64_t)OCC_FANIN, a.rec_len[r] - m + 1 - w0);   // >= 1: the block exists
        const int need = nw + m - 1;                               // codes of the block, all inside the record
        const int64_t s0 = a.rec_off[r] + w0;
        for (int i = w; i < EXP_CS; i += OCC_FANIN) {
            uint8_t c = EXP_FOREIGN;
            if (i < need) {
                const uint8_t x = a.codes[s0 + i] & 7u;
                if ((int)x < nl) c = x;
            }
            cl[j][i] = c;
        }
    }
    __syncthreads();
    bool has = live && w < nw;                                     // this lane's window has a term
    if (has)
        for (int k = 0; k < m; ++k) has = has && cl[j][w + k] != EXP_FOREIGN;
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

// rec_off / rec_len: HOST copies, already checked; d_rec_off / d_rec_len: the same on the device.  Launches on st, does not wait.
static int exp_run(pfmscan_ctx *ctx, const char *who, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                   const uint8_t *d_codes, int64_t n_pos, const int64_t *rec_off, const int64_t *rec_len, const int64_t *d_rec_off,
                   const int64_t *d_rec_len, int64_t n_rec, double *d_exp, double *d_occ, int64_t *d_windows, hipStream_t st)
{
    int rc;
    const bool posterior = mode == PFMSCAN_EXPECT_POSTERIOR;
    const int64_t pairs = n_rec * n_motifs;
    const int64_t n_col = (int64_t)n_motifs * m * n_letters;
    if (n_col > (int64_t(1) << 30)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many motifs for one call");
    // the occupancy of the same records first: v of posterior mode, and what the caller asked for
    if (posterior || d_occ || d_windows) {
        if (!d_occ) {
            if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
            d_occ = (double *)ctx->exp_occ.p;
        }
        if ((rc = occ_run_letters(ctx, who, ratio_tables, n_motifs, m, n_letters, d_codes, n_pos, rec_off, rec_len, d_rec_off, d_rec_len, n_rec,
                                  d_occ, d_windows, st)))
            return rc;
    }
    const double *d_inv = nullptr;
    if (posterior) {
        if ((rc = ensure(ctx, ctx->exp_inv, (size_t)pairs * 8))) return rc;
        if ((rc = exp_launch_inverse(ctx, d_occ, (double *)ctx->exp_inv.p, pairs, st))) return rc;
        d_inv = (const double *)ctx->exp_inv.p;
    }
    // the columns >= n_letters of every matrix row are +0.0; every other cell is written by k_occ_finish
    HIP_TRY(ctx, hipMemsetAsync(d_exp, 0, (size_t)pairs * m * 8 * sizeof(double), st));
    std::vector<int64_t> start(2 * (size_t)(n_rec + 1));
    int64_t *blk = start.data(), *grp = blk + n_rec + 1;
    int64_t max_blk = 0;
    blk[0] = grp[0] = 0;
    for (int64_t r = 0; r < n_rec; ++r) {
        const int64_t nw = std::max<int64_t>(rec_len[r] - m + 1, 0), nb = (nw + OCC_FANIN - 1) / OCC_FANIN;
        blk[r + 1] = blk[r] + nb;
        grp[r + 1] = grp[r] + (nb + OCC_FANIN - 1) / OCC_FANIN;
        max_blk = std::max(max_blk, nb);
    }
    const int64_t cap = occ_scratch_cap();
    // columns per pass: all of them unless the longest record's block sums alone pass the cap; then records per pass
    const int n_c_max = (int)std::min<int64_t>(n_col, std::max<int64_t>(1, cap / std::max<int64_t>(max_blk, 1)));
    const int64_t blk_cap = std::max<int64_t>(cap / n_c_max, 1), rec_cap = std::max<int64_t>((int64_t(1) << 30) / n_c_max, 1);
    std::vector<int64_t> cuts(1, 0);
    int64_t need_blk = 0, need_grp = 0;
    for (int64_t r0 = 0; r0 < n_rec;) {
        int64_t r1 = r0 + 1;
        while (r1 < n_rec && r1 - r0 < rec_cap && blk[r1 + 1] - blk[r0] <= blk_cap) ++r1;
        cuts.push_back(r1);
        need_blk = std::max(need_blk, blk[r1] - blk[r0]);
        need_grp = std::max(need_grp, grp[r1] - grp[r0]);
        r0 = r1;
    }
    if ((need_blk + EXP_WB - 1) / EXP_WB > 0x7FFFFFFF) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": a record is too long for one call");
    const size_t tab_bytes = (size_t)n_motifs * m * 8 * sizeof(double);
    if ((rc = ensure(ctx, ctx->occ_tab, tab_bytes))) return rc;
    if ((rc = ensure(ctx, ctx->occ_idx, start.size() * 8))) return rc;
    if ((rc = ensure(ctx, ctx->occ_bs, std::max<size_t>((size_t)need_blk * n_c_max * 8, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->occ_gs, std::max<size_t>((size_t)need_grp * n_c_max * 8, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->occ_cnt, std::max<size_t>((size_t)((need_blk + EXP_WB - 1) / EXP_WB) * 8, 16)))) return rc;   // a pass's workgroup -> record
    int64_t *wg_rec = (int64_t *)ctx->occ_cnt.p;
    if ((rc = upload(ctx, ctx->occ_tab.p, ratio_tables, tab_bytes, st))) return rc;
    if ((rc = upload(ctx, ctx->occ_idx.p, start.data(), start.size() * 8, st))) return rc;
    OccArgs a{};
    a.codes = d_codes;
    a.n_pos = n_pos;
    a.rec_off = d_rec_off;
    a.rec_len = d_rec_len;
    a.blk_start = (const int64_t *)ctx->occ_idx.p;
    a.grp_start = a.blk_start + n_rec + 1;
    a.tables = (const double *)ctx->occ_tab.p;
    a.m = m;
    a.n_letters = n_letters;
    a.n_motifs = n_motifs;
    a.bs = (double *)ctx->occ_bs.p;
    a.gs = (double *)ctx->occ_gs.p;
    a.occ = d_exp;
    a.out_stride = (int64_t)n_motifs * m * 8;
    a.cell_nl = n_letters;
    for (int64_t c0 = 0; c0 < n_col; c0 += n_c_max) {
        a.q_first = (int)c0;
        a.n_q = (int)std::min<int64_t>(n_c_max, n_col - c0);
        for (size_t i = 0; i + 1 < cuts.size(); ++i) {
            const bool make_table = cuts.size() > 2 || c0 == 0;    // one range of records: its table is made once, for all passes over the columns
            a.r0 = cuts[i];
            a.r1 = cuts[i + 1];
            a.blk_base = blk[a.r0];
            a.n_blk = blk[a.r1] - a.blk_base;
            a.grp_base = grp[a.r0];
            a.n_grp = grp[a.r1] - a.grp_base;
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
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the record table decides every address the kernels form: it is read back and checked before anything is launched
    std::vector<int64_t> rec(2 * (size_t)n_rec);
    HIP_TRY(ctx, hipMemcpyAsync(rec.data(), d_rec_off, (size_t)n_rec * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rec.data() + n_rec, d_rec_len, (size_t)n_rec * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = occ_check_records(ctx, who, rec.data(), rec.data() + n_rec, n_rec, n_pos)) return rc;
    return exp_run(ctx, who, ratio_tables, n_motifs, m, n_letters, mode, d_codes, n_pos, rec.data(), rec.data() + n_rec, d_rec_off, d_rec_len,
                   n_rec, d_exp, d_occ, d_windows, ctx->stream);
}

int pfmscan_expect_staged(pfmscan_ctx *ctx, int which, const double *ratio_tables, int n_motifs, int m, int n_letters, int mode,
                          const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *exp, double *occ, int64_t *windows)
{
    const char *who = "pfmscan_expect_staged";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (which != 0 && which != 1) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": which must be 0 (codes) or 1 (codes2)");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && !(which ? ctx->staged_codes2 : ctx->staged_codes))
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + (which ? ": no codes2 are staged (pfmscan_stage_codes2)" : ": no codes are staged"));
    const int64_t n_pos = ctx->staged_n;
    if (int rc = occ_check(ctx, who, ratio_tables, n_motifs, m, n_letters, n_pos, n_rec)) return rc;
    if (int rc = exp_check_mode(ctx, who, mode)) return rc;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len || !exp) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or output");
    if (int rc = occ_check_records(ctx, who, rec_off, rec_len, n_rec, n_pos)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t pairs = (size_t)n_rec * n_motifs, cells = pairs * m * 8;
    if ((rc = ensure(ctx, ctx->occ_rec, (size_t)n_rec * 16))) return rc;
    if ((rc = ensure(ctx, ctx->exp_out, (cells + pairs + (size_t)n_rec) * 8))) return rc;
    int64_t *d_off = (int64_t *)ctx->occ_rec.p, *d_len = d_off + n_rec;
    if ((rc = upload(ctx, d_off, rec_off, (size_t)n_rec * 8, ctx->stream))) return rc;
    if ((rc = upload(ctx, d_len, rec_len, (size_t)n_rec * 8, ctx->stream))) return rc;
    double *d_exp = (double *)ctx->exp_out.p;
    double *d_occ = occ ? d_exp + cells : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_exp + cells + pairs) : nullptr;
    const uint8_t *d_codes = (const uint8_t *)(which ? ctx->codes2.p : ctx->codes.p);
    if ((rc = exp_run(ctx, who, ratio_tables, n_motifs, m, n_letters, mode, d_codes, n_pos, rec_off, rec_len, d_off, d_len, n_rec, d_exp, d_occ,
                      d_win, ctx->stream)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(exp, d_exp, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (occ) HIP_TRY(ctx, hipMemcpyAsync(occ, d_occ, pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (windows) HIP_TRY(ctx, hipMemcpyAsync(windows, d_win, (size_t)n_rec * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFMSCAN_OK;
}

}  // extern "C"
