// pfmscan_footprint_profile.hip -- the posterior site map on averaged-structure profiles: the weight of every window and the
// coverage of every position of a profile record (DESIGN.md 5l "on averaged-structure profiles", include/pfmscan.h "posterior
// site map on averaged-structure profiles").
//
// The term t_s of a window and whether it has one are those of the occupancy on profiles (k_occ_profile_blocks): the chain of
// marginals (occp_marginal, one definition) under the structure tables, in joint mode behind the letter chain of the sequence
// tables; a window that holds a code >= 4 has no term.  The weight is that of the expected counts on profiles (k_expp_blocks):
// the term, or t_s * v with v = 1.0 / occ_r, and every weight +0.0 when occ_r == 0.0 -- decided on occ itself, never on the
// sign of v: negative profile cells are legal, and with them a negative occupancy.  The maps are those of pfmscan_footprint.hip:
// start[q][off_r + s] = w_s, cover[q][off_r + i] = the m weights of the windows over i added in ascending s from +0.0, every
// addition rounded and all m of them made (a weight can be -0.0 or negative here: nothing is skipped, nothing slides).
// No transcendental, no atomics on doubles, no tolerance: tests/footprint_profile_rules.py restates it and the bits are compared.
//
// The occupancy of the call is made first by the occupancy's own code over the same records (occ_run with the profile) and
// inverted by k_exp_inverse, as the expected counts do it.  Then k_occ_run_records writes the record of every tile (no
// workgroup bisects a prefix table: 17 dependent loads in front of everything) and ONE level-0 kernel runs:
//   k_fp_profile_tiles<T, SEQ, EVENTS>
//                A workgroup owns FPP_SLOTS consecutive windows of ONE record: the last FPP_SLOTS - (m - 1) are its tile of
//                positions, the first m - 1 the halo before it, whose weights it makes again.  The rows under these windows are
//                fetched as the aligned 16-byte vectors that cover them (occp_load, the stream's last one cut short), clipped to
//                the record at BOTH ends, and parked in LDS as doubles; in joint mode the codes lie beside them as bytes, foreign
//                codes and what lies outside the record as 0xFF.  A slot whose window begins before the record or ends behind it
//                has no term by 0 <= s < n_win -- never by what was loaded.  Per motif a lane makes its window's chain and
//                weight (the table rows are workgroup-uniform: tables, planes and event buffers are separate __restrict__
//                arguments) and parks the weight in LDS; after a barrier a lane per position adds slots i .. i + m - 1 in
//                ascending order -- consecutive lanes read consecutive doubles -- and stores start and cover with coalesced
//                8-byte stores, or (EVENTS) queues the position in LDS when cover > thr.  The queue leaves through the
//                HitShard protocol with one returning atomic per workgroup and motif: k_fp_tiles' tail.
#include <algorithm>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_fp.hpp"
#include "pfmscan_fp_plan.hpp"
#include "pfmscan_occ.hpp"

#pragma clang fp contract(off)   // products and sums are rounded one operation at a time: never an FMA

namespace pfmscan {

#ifndef PFMSCAN_FPP_SLOTS                                          // an A/B build (tools/build_variant.sh) may try another geometry
#define PFMSCAN_FPP_SLOTS PFMSCAN_FOOTPRINT_PROFILE_SLOTS
#endif
constexpr int FPP_SLOTS = PFMSCAN_FPP_SLOTS;                       // windows of a workgroup
constexpr int FPP_WPL = FPP_SLOTS / BLOCK;                         // windows (and positions) of a lane
constexpr int FPP_ROWS = FPP_SLOTS + PFMSCAN_MAX_M - 1;            // rows it stages at most
constexpr int FPP_CS = (FPP_ROWS + 7) / 8 * 8;                     // bytes of the strip of codes
constexpr uint8_t FPP_FOREIGN = 0xFF;
static_assert(FPP_WPL * BLOCK == FPP_SLOTS && FPP_WPL >= 1 && FPP_SLOTS > PFMSCAN_MAX_M - 1, "whole lanes, and a tile of at least one position");
static_assert(FPP_SLOTS <= 65536, "a queued position is 16 bits");

struct FppArgs {
    const int64_t *rec_off, *rec_len;   // [n_rec]
    const int64_t *tile_start;   // [n_rec + 1] prefix of ceil(L / tile)
    const int64_t *tile_rec;     // [n_tiles] the record of every tile (k_occ_run_records)
    int64_t n_pos;
    int m, n_motifs;
    int tile;                    // FPP_SLOTS - (m - 1)
    bool posterior;
    double thr;                  // events
    int64_t capacity;
};

// the events of a tile under one motif wait here and leave with one returning atomic
struct FppQueue {
    unsigned long long base;     // the workgroup's first slot, thread 0 -> everybody
    double cover[FPP_SLOTS];
    uint16_t at[FPP_SLOTS];      // position - the tile's first
    int n;
};
struct FppNoQueue {};

template <typename T, bool SEQ, bool EVENTS>
__global__ __launch_bounds__(BLOCK) void k_fp_profile_tiles(const FppArgs a, const unsigned char *__restrict__ profile, const uint8_t *__restrict__ codes,
                                                            const double *__restrict__ stab, const double *__restrict__ ltab,
                                                            const double *__restrict__ occ, const double *__restrict__ inv,
                                                            double *__restrict__ start, double *__restrict__ cover, int64_t *__restrict__ ev_key,
                                                            double *__restrict__ ev_cover, double *__restrict__ ev_start,
                                                            unsigned long long *__restrict__ ev_count)
{
    constexpr int RB = 7 * (int)sizeof(T);                         // bytes of a row
    constexpr int PER = 16 / (int)sizeof(T);                       // cells of a vector
    __shared__ double rows[FPP_ROWS * 7];
    __shared__ double wl[FPP_SLOTS];
    __shared__ uint8_t cl[SEQ ? FPP_CS : 8];
    __shared__ std::conditional_t<EVENTS, FppQueue, FppNoQueue> qu;
    const int t = threadIdx.x, m = a.m;
    const int64_t r = a.tile_rec[blockIdx.x];
    const int64_t L = a.rec_len[r], off = a.rec_off[r];
    const int64_t n_win = L - m + 1;                               // may be <= 0: a record shorter than the motif has positions, no window
    const int64_t t0 = ((int64_t)blockIdx.x - a.tile_start[r]) * a.tile;   // the tile's first position, within the record
    const int n_tp = (int)min((int64_t)a.tile, L - t0);            // its positions, >= 1: the tile exists
    const int64_t w0 = t0 - (m - 1);                               // the window of slot 0 and the row of LDS row 0: may be < 0
    const int n_slot = n_tp + m - 1;                               // slots that matter
    {
        // the rows of the record under these slots: [lo, hi) of the record, clipped at both ends; row x lies at LDS row x - w0
        const int64_t lo = max(w0, (int64_t)0), hi = min(w0 + n_slot + m - 1, L);   // lo <= t0 < hi
        const int nrows = (int)(hi - lo), lds0 = (int)(lo - w0) * 7;
        const int64_t first = (off + lo) * RB, end = first + (int64_t)nrows * RB, base = first & ~(int64_t)15, total = a.n_pos * RB;
        const int shift = (int)(first - base) / (int)sizeof(T);
        const int ncell = nrows * 7, nvec = (int)((end - base + 15) / 16);
        for (int v = t; v < nvec; v += BLOCK) {
            double d[PER];
            occp_cells(occp_load(profile, base + (int64_t)v * 16, total), d, T());
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int idx = v * PER + j - shift;
                if (idx >= 0 && idx < ncell) rows[lds0 + idx] = d[j];
            }
        }
        if constexpr (SEQ)
            for (int i = t; i < FPP_CS; i += BLOCK) {
                const int64_t x = w0 + i;
                uint8_t c = FPP_FOREIGN;
                if (i < n_slot + m - 1 && x >= 0 && x < L) {       // inside the record: inside the stream
                    c = codes[off + x] & 7u;
                    if (c >= 4u) c = FPP_FOREIGN;
                }
                cl[i] = c;
            }
    }
    __syncthreads();
    // a slot has a term when its window is one of the record's, and in joint mode holds no foreign code
    bool has[FPP_WPL];
#pragma unroll
    for (int j = 0; j < FPP_WPL; ++j) {
        const int s = t + j * BLOCK;
        const int64_t w = w0 + s;
        bool h = s < n_slot && w >= 0 && w < n_win;
        if constexpr (SEQ) {
            if (h)
                for (int k = 0; k < m; ++k) h = h && cl[s + k] != FPP_FOREIGN;
        }
        has[j] = h;
    }
    const int64_t p0 = off + t0;                                   // the tile's first position, in the stream
    const int64_t ms = (int64_t)m * 7, ml = (int64_t)m * 8;
    for (int q = 0; q < a.n_motifs; ++q) {
        if (q != 0) __syncthreads();                               // the adders (and the queue) of the last motif are done
        if constexpr (EVENTS)
            if (t == 0) qu.n = 0;
        const double *sp = stab + q * ms;
        const int64_t pq = r * a.n_motifs + q;
        bool zero = false;
        double v = 1.0;
        if (a.posterior) {
            zero = occ[pq] == 0.0;                                 // on occ itself: v may be negative
            v = inv[pq];
        }
#pragma unroll
        for (int j = 0; j < FPP_WPL; ++j) {
            const int s = t + j * BLOCK;
            double wt = 0.0;
            if (has[j]) {
                double tt = 0.0;
                if constexpr (SEQ) {
                    const double *lt = ltab + q * ml;
                    tt = lt[cl[s]];
                    for (int k = 1; k < m; ++k) tt = tt * lt[k * 8 + cl[s + k]];
                }
                double x[7];
                const double *rw = rows + s * 7;
#pragma unroll
                for (int c = 0; c < 7; ++c) x[c] = rw[c];
                const double d = occp_marginal(x, sp);
                tt = SEQ ? tt * d : d;
                for (int k = 1; k < m; ++k) {
                    rw += 7;
#pragma unroll
                    for (int c = 0; c < 7; ++c) x[c] = rw[c];
                    tt = tt * occp_marginal(x, sp + k * 7);
                }
                if (a.posterior) tt = zero ? 0.0 : tt * v;
                wt = tt;
            }
            wl[s] = wt;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FPP_WPL; ++j) {
            const int i = t + j * BLOCK;                           // position i of the tile: its windows are slots i .. i + m - 1
            if (i < n_tp) {
                const double st = wl[i + m - 1];
                double c = 0.0;
                if (EVENTS || cover)
                    for (int d = 0; d < m; ++d) c = c + wl[i + d];  // all m additions from +0.0: a weight may be -0.0 or negative
                if constexpr (EVENTS) {
                    if (c > a.thr) {                               // strict: NaN never passes
                        const int z = atomicAdd(&qu.n, 1);         // LDS; at most n_tp <= FPP_SLOTS per motif
                        qu.at[z] = (uint16_t)i;
                        qu.cover[z] = c;
                    }
                } else {
                    const int64_t p = (int64_t)q * a.n_pos + p0 + i;
                    if (start) start[p] = st;
                    if (cover) cover[p] = c;
                }
            }
        }
        if constexpr (EVENTS) {
            __syncthreads();
            const int n = qu.n;
            if (n != 0) {                                          // uniform: read behind the barrier
                const HitShard shard{ev_count, 1, a.capacity};
                if (t == 0) qu.base = shard.reserve((unsigned long long)n);
                __syncthreads();
                const unsigned long long base = qu.base;
                for (int i = t; i < n; i += BLOCK) {
                    const unsigned long long slot = base + (unsigned long long)i;
                    if (shard.in_range(slot)) {                    // slots at or beyond the capacity are counted, never stored
                        const int at = qu.at[i];
                        ev_key[slot] = (int64_t)q * a.n_pos + p0 + at;
                        ev_cover[slot] = qu.cover[i];
                        ev_start[slot] = wl[at + m - 1];
                    }
                }
            }
        }
    }
}

template <typename T, bool SEQ>
static void fpp_launch_t(const FppArgs &a, const dim3 grid, const void *d_profile, const uint8_t *d_codes, const double *stab, const double *ltab,
                         const double *d_occ, const double *d_inv, const FpOut &o, hipStream_t st)
{
    const unsigned char *pf = (const unsigned char *)d_profile;
    if (o.events)
        hipLaunchKernelGGL((k_fp_profile_tiles<T, SEQ, true>), grid, dim3(BLOCK), 0, st, a, pf, d_codes, stab, ltab, d_occ, d_inv, o.start, o.cover, o.ev_key,
                           o.ev_cover, o.ev_start, o.ev_count);
    else
        hipLaunchKernelGGL((k_fp_profile_tiles<T, SEQ, false>), grid, dim3(BLOCK), 0, st, a, pf, d_codes, stab, ltab, d_occ, d_inv, o.start, o.cover, o.ev_key,
                           o.ev_cover, o.ev_start, o.ev_count);
}

// Launches on st, does not wait.  d_codes where seq_tables is.
static int fpp_run(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                   const uint8_t *d_codes, const void *d_profile, int dtype, const OccRecords &rec, const FpOut &o, double *d_occ, int64_t *d_windows,
                   hipStream_t st)
{
    int rc;
    const bool posterior = mode == PFMSCAN_EXPECT_POSTERIOR;
    const int64_t pairs = rec.n_rec * n_motifs;
    // the occupancy of the same records first: v of posterior mode, and what the caller asked for
    if (posterior || d_occ || d_windows) {
        if (!d_occ) {
            if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
            d_occ = (double *)ctx->exp_occ.p;
        }
        const OccProfile pf{struct_tables, d_profile, dtype};
        if ((rc = occ_run(ctx, who, seq_tables, n_motifs, m, 4, seq_tables ? d_codes : nullptr, rec, d_occ, d_windows, st, &pf))) return rc;
    }
    const double *d_inv = nullptr;
    if (posterior) {
        if ((rc = ensure(ctx, ctx->exp_inv, (size_t)pairs * 8))) return rc;
        if ((rc = exp_launch_inverse(ctx, d_occ, (double *)ctx->exp_inv.p, pairs, st))) return rc;
        d_inv = (const double *)ctx->exp_inv.p;
    }
    // the tiles of the records: ceil(L / tile) each, numbered in record order, and behind the prefix the record of every tile
    const int tile = FPP_SLOTS - (m - 1);
    std::vector<int64_t> tiles;
    const int64_t n_tiles = fp_tile_prefix(rec.len, rec.n_rec, tile, tiles);
    if (n_tiles == 0) return PFMSCAN_OK;
    if (n_tiles < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many positions for one call");
    // 8 bytes per tile behind the prefix.  n_tiles <= n_rec + n_pos / tile: the table is smaller than the record table plus 1 / 600
    // of a float32 profile of the same stream, so it is the stream the caller already holds that bounds it, not FP_MAX_TILES (the
    // grid's limit: 16 GB of table would take a stream of 2^31 records or 4 * 10^11 rows); room that is not there is PFMSCAN_E_OOM
    if ((rc = ensure(ctx, ctx->fp_idx, (tiles.size() + (size_t)n_tiles) * 8))) return rc;
    if ((rc = upload(ctx, ctx->fp_idx.p, tiles.data(), tiles.size() * 8, st))) return rc;
    OccArgs ra{};                                                  // k_occ_run_records over the tile prefix: a tile is a run of one pass
    ra.r0 = 0;
    ra.r1 = rec.n_rec;
    ra.run_start = (const int64_t *)ctx->fp_idx.p;
    ra.run_base = 0;
    ra.run_rec = (int64_t *)ctx->fp_idx.p + tiles.size();
    occ_launch_run_records(ra, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(ctx, e, "k_occ_run_records");
    const double *ltab, *stab;
    if ((rc = occ_upload_tables(ctx, seq_tables, struct_tables, (size_t)n_motifs * m * 7 * sizeof(double), n_motifs, m, st, ltab, stab))) return rc;
    FppArgs a{};
    a.rec_off = rec.d_off;
    a.rec_len = rec.d_len;
    a.tile_start = ra.run_start;
    a.tile_rec = ra.run_rec;
    a.n_pos = rec.n_pos;
    a.m = m;
    a.n_motifs = n_motifs;
    a.tile = tile;
    a.posterior = posterior;
    a.thr = o.thr;
    a.capacity = o.capacity;
    const dim3 grid((unsigned)n_tiles);
    if (dtype == PFMSCAN_PROFILE_F64) {
        if (seq_tables) fpp_launch_t<double, true>(a, grid, d_profile, d_codes, stab, ltab, d_occ, d_inv, o, st);
        else fpp_launch_t<double, false>(a, grid, d_profile, d_codes, stab, ltab, d_occ, d_inv, o, st);
    } else {
        if (seq_tables) fpp_launch_t<float, true>(a, grid, d_profile, d_codes, stab, ltab, d_occ, d_inv, o, st);
        else fpp_launch_t<float, false>(a, grid, d_profile, d_codes, stab, ltab, d_occ, d_inv, o, st);
    }
    e = hipGetLastError();
    return e != hipSuccess ? fail_hip(ctx, e, "k_fp_profile_tiles") : PFMSCAN_OK;
}

// the checks of all four entry points up to "n_rec == 0 or n_motifs == 0: nothing to do", in the order of pfmscan_expect_profile_*
static int fpp_check(pfmscan_ctx *ctx, const char *who, const double *struct_tables, int n_motifs, int m, int mode, int profile_dtype, int64_t n_pos,
                     int64_t n_rec)
{
    const char *own = profile_dtype != PFMSCAN_PROFILE_F32 && profile_dtype != PFMSCAN_PROFILE_F64 ? ": profile_dtype must be PFMSCAN_PROFILE_F32 or F64"
                      : mode != PFMSCAN_EXPECT_RATIO && mode != PFMSCAN_EXPECT_POSTERIOR       ? ": mode must be PFMSCAN_EXPECT_RATIO or PFMSCAN_EXPECT_POSTERIOR"
                                                                                               : nullptr;
    if (int rc = occ_check_base(ctx, who, m, own, n_motifs, n_rec, n_pos, nullptr)) return rc;
    if (!struct_tables)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": struct_tables is NULL (sequence weights over a profile's records are pfmscan_footprint_* on the codes)");
    return PFMSCAN_OK;
}

// both _dev forms
static int fpp_dev(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                   const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len,
                   int64_t n_rec, const FpOut &o, double *d_occ, int64_t *d_windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = fpp_check(ctx, who, struct_tables, n_motifs, m, mode, profile_dtype, n_pos, n_rec)) return rc;
    if (seq_tables && !d_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": seq_tables (joint mode) needs the codes");
    if (o.events) {
        if (int rc = fp_check_events(ctx, who, o.thr, o.capacity, o.ev_count, o.ev_key, o.ev_cover, o.ev_start)) return rc;
    } else if (!o.start && !o.cover) {
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": d_start and d_cover are both NULL");
    }
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || (n_pos > 0 && !d_profile)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or profile");
    if (misaligned(d_profile) || (seq_tables && misaligned(d_codes)))
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    return fpp_run(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, d_codes, d_profile, profile_dtype, rec, o, d_occ, d_windows, ctx->stream);
}

// the checks of both _staged forms, up to "n_rec == 0 or n_motifs == 0: nothing to do" without the outputs' own
static int fpp_staged_check(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                            int64_t n_rec)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (!ctx->staged_profile) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no profile is staged");
    if (seq_tables && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": seq_tables (joint mode) needs staged codes");
    return fpp_check(ctx, who, struct_tables, n_motifs, m, mode, ctx->staged_dtype, ctx->staged_n, n_rec);
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_footprint_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                  const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off,
                                  const int64_t *d_rec_len, int64_t n_rec, double *d_start, double *d_cover, double *d_occ, int64_t *d_windows)
{
    const FpOut o{d_start, d_cover, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    return fpp_dev(ctx, "pfmscan_footprint_profile_dev", struct_tables, seq_tables, n_motifs, m, mode, d_codes, d_profile, profile_dtype, n_pos, d_rec_off,
                   d_rec_len, n_rec, o, d_occ, d_windows);
}

int pfmscan_footprint_profile_events_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                         const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off,
                                         const int64_t *d_rec_len, int64_t n_rec, double thr, int64_t capacity, int64_t *d_ev_key,
                                         double *d_ev_cover, double *d_ev_start, uint64_t *d_ev_count, double *d_occ, int64_t *d_windows)
{
    const FpOut o{nullptr, nullptr, true, thr, capacity, d_ev_key, d_ev_cover, d_ev_start, reinterpret_cast<unsigned long long *>(d_ev_count)};
    return fpp_dev(ctx, "pfmscan_footprint_profile_events_dev", struct_tables, seq_tables, n_motifs, m, mode, d_codes, d_profile, profile_dtype, n_pos,
                   d_rec_off, d_rec_len, n_rec, o, d_occ, d_windows);
}

int pfmscan_footprint_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                     const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *start, double *cover, double *occ,
                                     int64_t *windows)
{
    const char *who = "pfmscan_footprint_profile_staged";
    if (int rc = fpp_staged_check(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, n_rec)) return rc;
    if (!start && !cover) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": start and cover are both NULL");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const int64_t n_pos = ctx->staged_n;
    const size_t plane = (size_t)n_motifs * (size_t)n_pos, pairs = (size_t)n_rec * n_motifs;
    if ((rc = ensure(ctx, ctx->fp_out, std::max<size_t>((2 * plane + pairs + (size_t)n_rec) * 8, 16)))) return rc;
    double *d_base = (double *)ctx->fp_out.p;
    double *d_start = start ? d_base : nullptr;
    double *d_cover = cover ? d_base + plane : nullptr;
    double *d_occ = occ ? d_base + 2 * plane : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_base + 2 * plane + pairs) : nullptr;
    // positions in no record of the table are +0.0
    if (d_start && plane) HIP_TRY(ctx, hipMemsetAsync(d_start, 0, plane * 8, ctx->stream));
    if (d_cover && plane) HIP_TRY(ctx, hipMemsetAsync(d_cover, 0, plane * 8, ctx->stream));
    const FpOut o{d_start, d_cover, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    if ((rc = fpp_run(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, (const uint8_t *)ctx->codes.p, ctx->profile.p, ctx->staged_dtype, rec, o, d_occ,
                      d_win, ctx->stream)))
        return rc;
    return occ_copy_home(ctx, {{start, d_start, plane * 8}, {cover, d_cover, plane * 8}, {occ, d_occ, pairs * 8}, {windows, d_win, (size_t)n_rec * 8}});
}

int pfmscan_footprint_profile_events_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int mode,
                                            const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double thr, int64_t capacity,
                                            int64_t *ev_key, double *ev_cover, double *ev_start, int64_t *n_events, double *occ, int64_t *windows)
{
    const char *who = "pfmscan_footprint_profile_events_staged";
    if (int rc = fpp_staged_check(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, n_rec)) return rc;
    if (int rc = fp_check_events(ctx, who, thr, capacity, n_events, ev_key, ev_cover, ev_start)) return rc;
    *n_events = 0;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const size_t pairs = (size_t)n_rec * n_motifs;
    FpOut o;
    double *d_occ;
    int64_t *d_win;
    if ((rc = fp_events_room(ctx, thr, capacity, pairs, (size_t)n_rec, occ != nullptr, windows != nullptr, o, d_occ, d_win))) return rc;
    if ((rc = fpp_run(ctx, who, struct_tables, seq_tables, n_motifs, m, mode, (const uint8_t *)ctx->codes.p, ctx->profile.p, ctx->staged_dtype, rec, o, d_occ,
                      d_win, ctx->stream)))
        return rc;
    return fp_events_home(ctx, who, o, ev_key, ev_cover, ev_start, n_events, {occ, d_occ, pairs * 8}, {windows, d_win, (size_t)n_rec * 8});
}

}  // extern "C"
