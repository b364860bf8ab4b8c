// pfmscan_footprint.hip -- the posterior site map: the weight of every window and the coverage of every position
// (include/pfmscan.h "posterior site map").
//
// The weight w_s of window s is the expected counts' (pfmscan_expect.hip): the occupancy's term, or that times v = 1.0 / occ_r.
// Here it is not summed away by letter: start[q][off_r + s] = w_s, and cover[q][off_r + i] is the sum of the at most m weights
// of the windows that lie over position i, added in ascending s from +0.0, every addition rounded.  No transcendental, no
// atomics on doubles, no tolerance: tests/footprint_rules.py restates it in numpy and the bits are compared.
//
// The occupancy of the call is made first by the occupancy's own code over the same records (occ_run) and inverted by
// k_exp_inverse, as the expected counts do it.  Then ONE level-0 kernel:
//   k_fp_tiles   A workgroup owns FP_SLOTS consecutive windows of ONE record: the last FP_SLOTS - (m - 1) of them are its tile
//                of positions, the first m - 1 the halo before it, whose weights it makes again instead of reading them back.
//                The strip(s) of codes under these windows are parked in LDS (foreign codes and what lies outside the record
//                as 0xFF).  A lane owns FP_WPL slots, t + j * 256: whether a slot's window has a term is decided once, then
//                for every motif of the call the tables are reloaded, the lane makes its windows' chains and parks the
//                weights in LDS (+0.0 without a term), and a lane per position adds its m weights in ascending order from
//                LDS -- consecutive lanes read consecutive doubles -- and stores start and cover with coalesced 8-byte
//                stores into the motif's plane, or (EVENTS) parks the position in an LDS queue when cover > thr.  The queue
//                leaves through the HitShard protocol with one returning atomic per workgroup and motif, as k_mutmap's does.
//                PAIR: two strips, two tables, the joint chain.  Nothing is indexed at run time but LDS.
// Two windows per lane: with one (a tile of 256 - (m - 1) positions) a quarter of the chains at m = 64 are halo; with two an
// eighth, at the same LDS per position.  Timed against one and four per lane (profiles/footprint/NOTES.md): one is the slowest
// at every width, four gains at w = 8 and 12 and loses at w = 64; two is never the worst and was kept.
// A workgroup finds its record by bisection of the tile prefix table (occ_record): the table is the only thing the host makes.
#include <algorithm>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_fp.hpp"
#include "pfmscan_occ.hpp"

#pragma clang fp contract(off)   // products and sums are rounded one operation at a time: never an FMA

namespace pfmscan {

#ifndef PFMSCAN_FP_SLOTS                                           // an A/B build (tools/build_variant.sh) may try another geometry
#define PFMSCAN_FP_SLOTS PFMSCAN_FOOTPRINT_SLOTS
#endif
constexpr int FP_SLOTS = PFMSCAN_FP_SLOTS;                         // windows of a workgroup
constexpr int FP_WPL = FP_SLOTS / BLOCK;                           // windows (and positions) of a lane
constexpr int FP_CS = (FP_SLOTS + PFMSCAN_MAX_M - 1 + 3) / 4 * 4;  // bytes of a strip of codes
constexpr uint8_t FP_FOREIGN = 0xFF;
static_assert(FP_WPL * BLOCK == FP_SLOTS && FP_WPL >= 1 && FP_SLOTS > PFMSCAN_MAX_M - 1, "whole lanes, and a tile of at least one position");
static_assert(FP_SLOTS <= 65536, "a queued position is 16 bits");

struct FpArgs {
    const uint8_t *codes;        // [n_pos] the first strip: RNA codes, or the structure-letter codes of a structure-only call
    const uint8_t *codes2;       // [n_pos] PAIR: structure-letter codes
    const double *tables;        // [n_motifs][m][8] device: the tables over codes
    const double *tables2;       // PAIR: the structure tables
    const int64_t *rec_off, *rec_len;   // [n_rec]
    const int64_t *tile_start;   // [n_rec + 1] prefix of ceil(L / tile)
    int64_t n_rec, n_pos;
    const double *inv;           // [n_rec][n_motifs] or null (ratio mode)
    int m, nl;                   // nl: letters of codes (4 or 7)
    int n_motifs;
    int tile;                    // FP_SLOTS - (m - 1)
    double *start, *cover;       // [n_motifs][n_pos], either may be null (maps)
    double thr;                  // events
    int64_t capacity;
    int64_t *ev_key;             // [capacity] q * n_pos + p
    double *ev_cover, *ev_start; // [capacity]
    unsigned long long *ev_count;
};

// the events of a tile under one motif wait here and leave with one returning atomic
struct FpQueue {
    unsigned long long base;     // the workgroup's first slot, thread 0 -> everybody
    double cover[FP_SLOTS];
    uint16_t at[FP_SLOTS];       // position - the tile's first
    int n;
};
struct FpNoQueue {};

template <bool PAIR, bool EVENTS>
__global__ __launch_bounds__(BLOCK) void k_fp_tiles(const FpArgs a)
{
    constexpr int NS = PAIR ? 2 : 1;
    __shared__ double tab[NS][PFMSCAN_MAX_M * 8];
    __shared__ double wl[FP_SLOTS];
    __shared__ uint8_t cl[NS][FP_CS];
    __shared__ std::conditional_t<EVENTS, FpQueue, FpNoQueue> qu;
    const int t = threadIdx.x, m = a.m;
    const int64_t r = occ_record(a.tile_start, 0, a.n_rec, (int64_t)blockIdx.x);
    const int64_t L = a.rec_len[r], off = a.rec_off[r];
    const int64_t t0 = ((int64_t)blockIdx.x - a.tile_start[r]) * a.tile;   // the tile's first position, within the record
    const int n_tp = (int)min((int64_t)a.tile, L - t0);            // its positions, >= 1: the tile exists
    const int64_t w0 = t0 - (m - 1);                               // the window of slot 0 and the position of strip byte 0: may be < 0
    const int n_byte = n_tp + 2 * (m - 1);                         // strip bytes under the slots that matter, <= FP_CS
    for (int i = t; i < FP_CS; i += BLOCK) {
        const int64_t x = w0 + i;
        uint8_t c0 = FP_FOREIGN, c1 = FP_FOREIGN;
        if (i < n_byte && x >= 0 && x < L) {                       // inside the record: inside the stream
            c0 = a.codes[off + x] & 7u;
            if ((int)c0 >= a.nl) c0 = FP_FOREIGN;
            if constexpr (PAIR) {
                c1 = a.codes2[off + x] & 7u;
                if ((int)c1 >= PFMSCAN_NSTRUCT) c1 = FP_FOREIGN;
            }
        }
        cl[0][i] = c0;
        if constexpr (PAIR) cl[1][i] = c1;
    }
    __syncthreads();
    // a window that begins before the record or ends behind it has a foreign byte under it: has is also 0 <= s < n_win
    bool has[FP_WPL];
#pragma unroll
    for (int j = 0; j < FP_WPL; ++j) {
        const int s = t + j * BLOCK;
        bool h = s < n_tp + m - 1;
        if (h)
            for (int k = 0; k < m; ++k) {
                h = h && cl[0][s + k] != FP_FOREIGN;
                if constexpr (PAIR) h = h && cl[1][s + k] != FP_FOREIGN;
            }
        has[j] = h;
    }
    const int64_t p0 = off + t0;                                   // the tile's first position, in the stream
    for (int q = 0; q < a.n_motifs; ++q) {
        if (q != 0) __syncthreads();                               // the adders (and the queue) of the last motif are done
        for (int i = t; i < m * 8; i += BLOCK) {
            tab[0][i] = a.tables[(int64_t)q * m * 8 + i];
            if constexpr (PAIR) tab[1][i] = a.tables2[(int64_t)q * m * 8 + i];
        }
        if constexpr (EVENTS)
            if (t == 0) qu.n = 0;
        __syncthreads();
        const double v = a.inv ? a.inv[r * a.n_motifs + q] : 1.0;
#pragma unroll
        for (int j = 0; j < FP_WPL; ++j) {
            const int s = t + j * BLOCK;
            double wt = 0.0;
            if (has[j]) {
                const uint8_t *cp = &cl[0][s];
                double x = tab[0][cp[0]];
                for (int k = 1; k < m; ++k) x = x * tab[0][k * 8 + cp[k]];
                if constexpr (PAIR) {
                    cp = &cl[1][s];
                    for (int k = 0; k < m; ++k) x = x * tab[1][k * 8 + cp[k]];
                }
                if (a.inv) x = v < 0.0 ? 0.0 : x * v;
                wt = x;
            }
            wl[s] = wt;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FP_WPL; ++j) {
            const int i = t + j * BLOCK;                           // position i of the tile: its windows are slots i .. i + m - 1
            if (i < n_tp) {
                const double st = wl[i + m - 1];
                double c = 0.0;
                if (EVENTS || a.cover)
                    for (int d = 0; d < m; ++d) c = c + wl[i + d];
                if constexpr (EVENTS) {
                    if (c > a.thr) {                               // strict: NaN never passes
                        const int z = atomicAdd(&qu.n, 1);         // LDS; at most n_tp <= FP_SLOTS per motif
                        qu.at[z] = (uint16_t)i;
                        qu.cover[z] = c;
                    }
                } else {
                    const int64_t p = (int64_t)q * a.n_pos + p0 + i;
                    if (a.start) a.start[p] = st;
                    if (a.cover) a.cover[p] = c;
                }
            }
        }
        if constexpr (EVENTS) {
            __syncthreads();
            const int n = qu.n;
            if (n != 0) {                                          // uniform: read behind the barrier
                const HitShard shard{a.ev_count, 1, a.capacity};
                if (t == 0) qu.base = shard.reserve((unsigned long long)n);
                __syncthreads();
                const unsigned long long base = qu.base;
                for (int i = t; i < n; i += BLOCK) {
                    const unsigned long long slot = base + (unsigned long long)i;
                    if (shard.in_range(slot)) {                    // slots at or beyond the capacity are counted, never stored
                        const int at = qu.at[i];
                        a.ev_key[slot] = (int64_t)q * a.n_pos + p0 + at;
                        a.ev_cover[slot] = qu.cover[i];
                        a.ev_start[slot] = wl[at + m - 1];
                    }
                }
            }
        }
    }
}

// Launches on st, does not wait.  At least one table is given; d_codes where seq_tables is, d_codes2 where struct_tables is.
static int fp_run(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                  const uint8_t *d_codes, const uint8_t *d_codes2, const OccRecords &rec, const FpOut &o, double *d_occ, int64_t *d_windows,
                  hipStream_t st)
{
    int rc;
    const bool posterior = mode == PFMSCAN_EXPECT_POSTERIOR, pair = seq_tables && struct_tables;
    const int64_t pairs = rec.n_rec * n_motifs;
    // one table: its stream is the first strip
    const double *tables = seq_tables ? seq_tables : struct_tables;
    const uint8_t *codes = seq_tables ? d_codes : d_codes2;
    const int nl = seq_tables ? 4 : PFMSCAN_NSTRUCT;
    // the occupancy of the same records first: v of posterior mode, and what the caller asked for
    if (posterior || d_occ || d_windows) {
        if (!d_occ) {
            if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
            d_occ = (double *)ctx->exp_occ.p;
        }
        const OccPair pr{struct_tables, d_codes2};
        if ((rc = occ_run(ctx, who, tables, n_motifs, m, nl, codes, rec, d_occ, d_windows, st, nullptr, pair ? &pr : nullptr))) return rc;
    }
    FpArgs a{};
    if (posterior) {
        if ((rc = ensure(ctx, ctx->exp_inv, (size_t)pairs * 8))) return rc;
        if ((rc = exp_launch_inverse(ctx, d_occ, (double *)ctx->exp_inv.p, pairs, st))) return rc;
        a.inv = (const double *)ctx->exp_inv.p;
    }
    // the tiles of the records: ceil(L / tile) each, numbered in record order
    const int tile = FP_SLOTS - (m - 1);
    std::vector<int64_t> tiles((size_t)rec.n_rec + 1, 0);
    for (int64_t r = 0; r < rec.n_rec; ++r) tiles[r + 1] = tiles[r] + (rec.len[r] + tile - 1) / tile;
    const int64_t n_tiles = tiles[rec.n_rec];
    if (n_tiles == 0) return PFMSCAN_OK;
    if (n_tiles > 0x7FFFFFFF) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many positions for one call");
    if ((rc = ensure(ctx, ctx->fp_idx, tiles.size() * 8))) return rc;
    if ((rc = upload(ctx, ctx->fp_idx.p, tiles.data(), tiles.size() * 8, st))) return rc;
    if ((rc = occ_upload_tables(ctx, tables, pair ? struct_tables : nullptr, (size_t)n_motifs * m * 8 * sizeof(double), n_motifs, m, st, a.tables,
                                a.tables2)))
        return rc;
    a.codes = codes;
    a.codes2 = pair ? d_codes2 : nullptr;
    a.rec_off = rec.d_off;
    a.rec_len = rec.d_len;
    a.tile_start = (const int64_t *)ctx->fp_idx.p;
    a.n_rec = rec.n_rec;
    a.n_pos = rec.n_pos;
    a.m = m;
    a.nl = nl;
    a.n_motifs = n_motifs;
    a.tile = tile;
    a.start = o.start;
    a.cover = o.cover;
    a.thr = o.thr;
    a.capacity = o.capacity;
    a.ev_key = o.ev_key;
    a.ev_cover = o.ev_cover;
    a.ev_start = o.ev_start;
    a.ev_count = o.ev_count;
    const dim3 grid((unsigned)n_tiles);
    if (pair) {
        if (o.events) hipLaunchKernelGGL((k_fp_tiles<true, true>), grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_fp_tiles<true, false>), grid, dim3(BLOCK), 0, st, a);
    } else {
        if (o.events) hipLaunchKernelGGL((k_fp_tiles<false, true>), grid, dim3(BLOCK), 0, st, a);
        else hipLaunchKernelGGL((k_fp_tiles<false, false>), grid, dim3(BLOCK), 0, st, a);
    }
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail_hip(ctx, e, "k_fp_tiles") : PFMSCAN_OK;
}

// the checks of all four entry points up to "n_rec == 0 or n_motifs == 0: nothing to do", in the order of pfmscan_expect_pair_*
static int fp_check(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                    int64_t n_pos, int64_t n_rec)
{
    if (int rc = occ_check_base(ctx, who, m, nullptr, n_motifs, n_rec, n_pos, seq_tables || struct_tables ? nullptr : ": seq_tables and struct_tables are both NULL"))
        return rc;
    if (mode != PFMSCAN_EXPECT_RATIO && mode != PFMSCAN_EXPECT_POSTERIOR)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": mode must be PFMSCAN_EXPECT_RATIO or PFMSCAN_EXPECT_POSTERIOR");
    return PFMSCAN_OK;
}

// both _dev forms
static int fp_dev(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                  const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec,
                  const FpOut &o, double *d_occ, int64_t *d_windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = fp_check(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, n_pos, n_rec)) return rc;
    if (o.events) {
        if (int rc = fp_check_events(ctx, who, o.thr, o.capacity, o.ev_count, o.ev_key, o.ev_cover, o.ev_start)) return rc;
    } else if (!o.start && !o.cover) {
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": d_start and d_cover are both NULL");
    }
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || (n_pos > 0 && ((seq_tables && !d_codes) || (struct_tables && !d_codes2))))
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or codes");
    if ((seq_tables && misaligned(d_codes)) || (struct_tables && misaligned(d_codes2)))
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    return fp_run(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, d_codes, d_codes2, rec, o, d_occ, d_windows, ctx->stream);
}

// the checks of both _staged forms of what is staged
static int fp_staged_check(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && seq_tables && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes are staged");
    if (ctx->staged_n > 0 && struct_tables && !ctx->staged_codes2)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes2 are staged (pfmscan_stage_codes2)");
    return PFMSCAN_OK;
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_footprint_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                          const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len,
                          int64_t n_rec, double *d_start, double *d_cover, double *d_occ, int64_t *d_windows)
{
    const FpOut o{d_start, d_cover, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    return fp_dev(ctx, "pfmscan_footprint_dev", seq_tables, struct_tables, n_motifs, m, mode, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, o,
                  d_occ, d_windows);
}

int pfmscan_footprint_events_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                                 const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                                 const int64_t *d_rec_len, int64_t n_rec, double thr, int64_t capacity, int64_t *d_ev_key, double *d_ev_cover,
                                 double *d_ev_start, uint64_t *d_ev_count, double *d_occ, int64_t *d_windows)
{
    const FpOut o{nullptr, nullptr, true, thr, capacity, d_ev_key, d_ev_cover, d_ev_start, reinterpret_cast<unsigned long long *>(d_ev_count)};
    return fp_dev(ctx, "pfmscan_footprint_events_dev", seq_tables, struct_tables, n_motifs, m, mode, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len,
                  n_rec, o, d_occ, d_windows);
}

int pfmscan_footprint_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                             const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double *start, double *cover, double *occ,
                             int64_t *windows)
{
    const char *who = "pfmscan_footprint_staged";
    if (int rc = fp_staged_check(ctx, who, seq_tables, struct_tables)) return rc;
    const int64_t n_pos = ctx->staged_n;
    if (int rc = fp_check(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, n_pos, n_rec)) return rc;
    if (!start && !cover) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": start and cover are both NULL");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
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
    if ((rc = fp_run(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, (const uint8_t *)ctx->codes.p, (const uint8_t *)ctx->codes2.p, rec, o, d_occ,
                     d_win, ctx->stream)))
        return rc;
    return occ_copy_home(ctx, {{start, d_start, plane * 8}, {cover, d_cover, plane * 8}, {occ, d_occ, pairs * 8}, {windows, d_win, (size_t)n_rec * 8}});
}

int pfmscan_footprint_events_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int mode,
                                    const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, double thr, int64_t capacity, int64_t *ev_key,
                                    double *ev_cover, double *ev_start, int64_t *n_events, double *occ, int64_t *windows)
{
    const char *who = "pfmscan_footprint_events_staged";
    if (int rc = fp_staged_check(ctx, who, seq_tables, struct_tables)) return rc;
    const int64_t n_pos = ctx->staged_n;
    if (int rc = fp_check(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, n_pos, n_rec)) return rc;
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
    if ((rc = fp_run(ctx, who, seq_tables, struct_tables, n_motifs, m, mode, (const uint8_t *)ctx->codes.p, (const uint8_t *)ctx->codes2.p, rec, o, d_occ,
                     d_win, ctx->stream)))
        return rc;
    return fp_events_home(ctx, who, o, ev_key, ev_cover, ev_start, n_events, {occ, d_occ, pairs * 8}, {windows, d_win, (size_t)n_rec * 8});
}

}  // extern "C"
