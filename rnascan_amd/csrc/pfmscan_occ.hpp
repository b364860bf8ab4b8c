// pfmscan_occ.hpp -- what the occupancy (pfmscan_occupancy.hip) and the expected counts (pfmscan_expect.hip,
// pfmscan_expect_profile.hip) share: the arguments of a pass and the frame every driver builds them with (the pass plan itself
// is pfmscan_occ_plan.hpp), the bisection of a prefix table, the host side of levels 1 and up of the summation tree, the
// pieces of the entry points (argument checks, the record table's way down and up, the copies home), and for
// averaged-structure profiles the geometry of a run, the loads of its rows and the marginal of a row (one definition:
// k_occ_profile_blocks and k_expp_blocks make the same bits of it).
#pragma once
#include <cstdint>
#include <initializer_list>

#include "pfmscan_ctx.hpp"
#include "pfmscan_occ_plan.hpp"

namespace pfmscan {

constexpr int64_t OCC_SCRATCH_DOUBLES = int64_t(1) << 25;   // block sums of one pass (256 MB); PFMSCAN_OCC_SCRATCH_DOUBLES overrides
static_assert(OCC_FANIN == PFMSCAN_OCC_FANIN && OCC_FANIN == 32, "a block is the 32 windows one lane walks; the masks are 32 bits wide");

struct OccArgs {
    const uint8_t *codes;        // [n_pos]
    int64_t n_pos;
    const int64_t *rec_off, *rec_len;   // [n_rec]
    const int64_t *blk_start;    // [n_rec + 1] prefix of ceil(n_win / 32)
    const int64_t *grp_start;    // [n_rec + 1] prefix of ceil(blocks / 32)
    int64_t r0, r1;              // records of this pass
    int64_t blk_base, n_blk;     // blk_start[r0], blocks of the pass
    int64_t grp_base, n_grp;
    const double *tables;        // [n_motifs][m][8] device
    int m, n_letters;
    int q_first, n_q;            // columns of this pass (n_q = row stride of the scratch): motifs, or cells of motifs (cell_nl)
    int chunk;                   // motifs per LDS chunk (gridDim.y chunks)
    int n_motifs;
    double *bs;                  // [n_blk][n_q] block sums
    double *gs;                  // [n_grp][n_q] level-1 sums, folded in place by k_occ_finish
    int *bcnt;                   // [n_blk] windows with a term, or null
    int *gcnt;                   // [n_grp]
    double *occ;                 // [n_rec][out_stride]: column q_first + q of record r, see cell_nl
    int64_t out_stride;          // doubles per record of occ
    int cell_nl;                 // 0: column x is stored at x.  n_letters: column x = row * n_letters + c is stored at row * 8 + c
    int64_t *windows;            // [n_rec] or null
    // averaged-structure profiles (k_occ_profile_blocks)
    const unsigned char *profile;   // [n_pos][7] float or double, 16-byte aligned
    const int64_t *run_start;    // [n_rec + 1] prefix of ceil(blocks / OCCP_RUN)
    int64_t run_base;            // run_start[r0]
    int64_t *run_rec;            // [runs of the pass] the record of every run (k_occ_run_records)
    // two code streams (k_occ_blocks<QN, true>, k_exp_pair_blocks): codes are the RNA codes, tables the sequence tables
    const uint8_t *codes2;       // [n_pos] structure-letter codes
    const double *tables2;       // [n_motifs][m][8] device: the structure tables of the pairs
};

// the record of element e of a prefix table: the last r in [r0, r1) with start[r] <= e (start[r1] > e)
__device__ __forceinline__ int64_t occ_record(const int64_t *__restrict__ start, int64_t r0, int64_t r1, int64_t e)
{
    int64_t lo = r0 + 1, hi = r1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (start[mid] > e) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

// ---- averaged-structure profiles: what the level-0 kernels of both files share -----------------------------------------
constexpr int OCCP_WIN = OCCP_RUN * OCC_FANIN;                     // its windows: a lane each
constexpr int OCCP_ROWS = OCCP_WIN + PFMSCAN_MAX_M - 1;            // rows it stages at most
constexpr int OCCP_TS = OCCP_RUN * (OCC_FANIN + 1);                // doubles of one motif's terms in LDS: window w at w + w / 32
constexpr int OCCP_CHUNK = 32;                                     // motifs a workgroup walks over the rows it staged
static_assert(OCCP_WIN == BLOCK, "a lane per window of the run");

// the aligned 16 bytes at byte_off; the stream's last vector may be cut short (rows are a multiple of 4 bytes)
__device__ __forceinline__ uint4 occp_load(const unsigned char *__restrict__ base, int64_t byte_off, int64_t total_bytes)
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

// the cells of one 16-byte vector, widened (exact)
__device__ __forceinline__ void occp_cells(const uint4 v, double (&d)[4], float)
{
    d[0] = (double)__uint_as_float(v.x);
    d[1] = (double)__uint_as_float(v.y);
    d[2] = (double)__uint_as_float(v.z);
    d[3] = (double)__uint_as_float(v.w);
}
__device__ __forceinline__ void occp_cells(const uint4 v, double (&d)[2], double)
{
    d[0] = __hiloint2double((int)v.y, (int)v.x);
    d[1] = __hiloint2double((int)v.w, (int)v.z);
}

// the marginal of row x under table row s: 7 rounded products, 6 rounded additions, ascending.  Every file that includes
// this header compiles under `#pragma clang fp contract(off)`: nothing here is fused.
__device__ __forceinline__ double occp_marginal(const double (&x)[7], const double *__restrict__ s)
{
#pragma clang fp contract(off)
    double d = x[0] * s[0];
#pragma unroll
    for (int c = 1; c < 7; ++c) d = d + x[c] * s[c];
    return d;
}

// what level 0 reads when the stream is an averaged-structure profile: its rows and the structure tables (HOST double
// [n_motifs][m][7]); the letter tables and the codes are then those of joint mode, or null
struct OccProfile {
    const double *struct_tables;
    const void *d_profile;
    int dtype;
};

// the record table of a call: HOST copies, already checked (ascending, disjoint, inside [0, n_pos)), and the same on the device
struct OccRecords {
    const int64_t *off, *len;
    const int64_t *d_off, *d_len;
    int64_t n_rec, n_pos;
};

// ---- pfmscan_occupancy.hip: the frame of a driver (occ_run, exp_run, exp_pair_run, expp_run) ------------------------------
// the scratch cap in doubles: OCC_SCRATCH_DOUBLES unless the environment says otherwise
int64_t occ_scratch_cap();
// The tables of a call on st: the letter tables (HOST double [n_motifs][m][8], or null) into ctx->occ_tab, then the structure
// tables (stab_bytes of them, or null) behind them.  d_tab: where the former lie (null when there are none), d_stab: the latter.
int occ_upload_tables(pfmscan_ctx *ctx, const double *letter_tables, const double *struct_tables, size_t stab_bytes, int n_motifs, int m,
                      hipStream_t st, const double *&d_tab, const double *&d_stab);
// Room for the block and level-1 sums of the plan's largest pass (`cells` doubles per unit and block), the plan's prefix tables
// uploaded on st (room for a pass's run -> record table behind them when it numbers runs), and the record-independent fields
// of the arguments: the streams' sizes, the record and prefix tables, run_rec, bs, gs, m, n_letters, n_motifs.
int occ_frame(pfmscan_ctx *ctx, const OccPlan &p, int cells, const OccRecords &rec, int n_motifs, int m, int n_letters, hipStream_t st, OccArgs &a);
// the fields of pass i of the plan: r0, r1, blk_base, n_blk, grp_base, n_grp, run_base; returns the runs of the pass
int64_t occ_set_pass(OccArgs &a, const OccPlan &p, size_t i);
// k_occ_run_records on st: the record of every run of the pass a describes (a.run_rec, from a.run_start / a.run_base over
// records a.r0 .. a.r1)
void occ_launch_run_records(const OccArgs &a, hipStream_t st);
// Levels 1 and up of a pass whose block sums lie in a.bs: k_occ_level1 (when the pass has blocks)
// and k_occ_finish on st; n_q independent columns per record, one writer per cell of a.occ.
int occ_launch_upper(pfmscan_ctx *ctx, const OccArgs &a, hipStream_t st);

// ---- pfmscan_occupancy.hip: the pieces of the entry points -----------------------------------------------------------------
// The checks every entry point of the family makes before the rule "n_rec == 0 or n_motifs == 0: nothing to do", in their
// order: the width; the caller's own test of its kind, mode or n_letters (own: what to say when it failed, else null); the
// sizes; a table that is NULL while there are motifs (missing: what to say, else null).
int occ_check_base(pfmscan_ctx *ctx, const char *who, int m, const char *own, int n_motifs, int64_t n_rec, int64_t n_pos, const char *missing);
int occ_check(pfmscan_ctx *ctx, const char *who, const double *ratio_tables, int n_motifs, int m, int n_letters, int64_t n_pos, int64_t n_rec);
// the checks the four two-stream entry points share
int occ_pair_check(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int64_t n_pos,
                   int64_t n_rec);
// A _dev form's record table: it decides every address the kernels form, so it is read back (into host; one synchronisation of
// ctx->stream) and checked before anything is launched.
int occ_records_home(pfmscan_ctx *ctx, const char *who, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, int64_t n_pos,
                     std::vector<int64_t> &host, OccRecords &rec);
// A _staged form's record table: checked, then uploaded into ctx->occ_rec on ctx->stream.
int occ_records_up(pfmscan_ctx *ctx, const char *who, const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, OccRecords &rec);
// the tail of a _staged form: every array that is asked for (dst not null) comes home on ctx->stream, one synchronisation
struct OccHome {
    void *dst;
    const void *d_src;
    size_t bytes;
};
int occ_copy_home(pfmscan_ctx *ctx, std::initializer_list<OccHome> arrays);

// ---- pfmscan_occupancy.hip: the occupancy itself, on st, without waiting ---------------------------------------------------
// the second stream of two code streams: pair q is (ratio_tables[q], struct_tables[q])
struct OccPair {
    const double *struct_tables;   // HOST double [n_motifs][m][8]
    const uint8_t *d_codes2;
};
// pf and pr null: letter strings (ratio_tables over d_codes).  pf: an averaged-structure profile, and ratio_tables / d_codes are
// the letter part of joint mode (n_letters 4) or null.  pr: two code streams, ratio_tables / d_codes the sequence side
// (n_letters 4).  Only the level-0 launch differs.
int occ_run(pfmscan_ctx *ctx, const char *who, const double *ratio_tables, int n_motifs, int m, int n_letters, const uint8_t *d_codes,
            const OccRecords &rec, double *d_occ, int64_t *d_windows, hipStream_t st, const OccProfile *pf = nullptr, const OccPair *pr = nullptr);
// pfmscan_expect.hip.  k_exp_inverse on st: inv[i] = 1.0 / occ[i], one rounded division each; -1.0 where occ[i] == 0.0
int exp_launch_inverse(pfmscan_ctx *ctx, const double *d_occ, double *d_inv, int64_t n, hipStream_t st);
// pfmscan_expect_merge.hip.  One matrix of a merged _staged form: the per-record matrices d_exp [n_rec][n_motifs][rows][8] a pass
// left on the device (null: this matrix is not asked for) and where its sums go on the HOST.
struct ExpMergeOut {
    const double *d_exp;
    uint64_t *acc;               // [n_motifs][PFMSCAN_SITE_LIMBS][rows * 8] normalised: this call's sums are ADDED
    int64_t *bad;                // [n_motifs][2] of this call
    int rows;                    // matrix rows of a motif: the width m, or 4 m for the letter-pair table of two code streams
};
// The tail of a merged _staged form, after its pass was launched on ctx->stream: k_exp_merge over every matrix that is asked for
// into ctx->exp_acc, then the accumulators, the verdicts, the occupancy and the window counts (null: not asked for) come home,
// one synchronisation, and the sums are added into out[i].acc (pfmscan_site_acc_add).
int exp_merge_home(pfmscan_ctx *ctx, const char *who, const ExpMergeOut *out, int n_out, int64_t n_rec, int n_motifs, int m, const double *d_occ,
                   double *occ, const int64_t *d_windows, int64_t *windows);

}  // namespace pfmscan
