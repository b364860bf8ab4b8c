// pfmscan_mutocc.hip -- threshold-free mutagenesis: what every single-letter change does to the summed likelihood ratio of the
// windows over its position (include/pfmscan.h "threshold-free mutagenesis").
//
// local[q][p][a] for a position p = off_r + i of record r that holds a letter, and a letter a: x = +0.0, then for the windows
// s = i - m + 1 .. i ascending x = x + u(s), every addition rounded; u(s) is the occupancy's term of window s with a written at
// i -- R[0][.], then * R[k][.] for k ascending, every product rounded -- or +0.0 where the window leaves the record or holds a
// foreign code at another position.  The column of the letter the record holds is the cover of pfmscan_footprint_* in ratio
// mode, bit for bit; tests/mutocc_rules.py restates the rule in numpy and the bits are compared.
//
// The products are sequential, so for the offset j = i - s the first j factors of a window do not depend on a: as in k_mutmap
// they are taken ONCE and shared by the four letters, the tail k > j is multiplied per letter, left to right (no suffix
// product: the bits would differ).
//
//   k_mutocc<M, EVENTS>        width as a compile-time constant (1 .. MO_FIXED_MAX): the 2M - 1 codes around a position sit in
//                              registers indexed by constants only (static_for), R[j][a] of the substituted letter is a
//                              scalar operand
//   k_mutocc_rolled<EVENTS>    any width up to PFMSCAN_MAX_M: the neighbourhood stays in LDS and is indexed there
// A workgroup owns a tile of MO_TILE positions of ONE record (occ_r, which the events compare with, is per record) and finds
// the record by bisection of the tile prefix table (occ_record).  The codes under the windows over the tile -- m - 1 bytes of
// halo on both sides -- are parked in LDS, foreign codes and what lies outside the record as 0xFF; whether a window has a
// term is decided once per tile; then the call's motifs are walked with the table in LDS.
//   dense   local double [n_motifs][n_pos][4] as two 16-byte stores per position; four NaN where the record holds no letter
//   EVENTS  nothing dense: delta = local[a] - local[c_i] (one rounded subtraction) against lim = frac * occ_r (one rounded
//           product), gain when delta > lim, loss when delta < -lim, both strict; the events of a tile under one motif wait in
//           LDS and leave through the HitShard protocol with one returning atomic per workgroup and motif
// The occupancy of the call is made first by the occupancy's own code (occ_run), as pfmscan_footprint.hip does it.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_fp.hpp"
#include "pfmscan_fp_plan.hpp"
#include "pfmscan_occ.hpp"

#pragma clang fp contract(off)   // products and sums are rounded one operation at a time: never an FMA

namespace pfmscan {

constexpr int MO_TILE = PFMSCAN_MUTOCC_TILE;                       // positions of a workgroup
constexpr int MO_PPL = MO_TILE / BLOCK;                            // positions of a lane
constexpr int MO_HALO = PFMSCAN_MAX_M - 1;                         // bytes before and behind the tile, at most
constexpr int MO_SLOTS = MO_TILE + MO_HALO;                        // windows over a tile, at most
constexpr int MO_CS = (MO_TILE + 2 * MO_HALO + 3) / 4 * 4;         // bytes of the strip of codes
constexpr int MO_FIXED_MAX = 20;                                   // widest compile-time instantiation, as k_mutmap's
constexpr uint8_t MO_FOREIGN = 0xFF;
static_assert(MO_PPL * BLOCK == MO_TILE && MO_PPL >= 1, "whole lanes");
static_assert(4 * MO_TILE <= 65536, "a queued event is 16 bits: 4 * (position - the tile's first) + letter");

struct MoArgs {
    const uint8_t *codes;        // [n_pos] RNA codes
    const double *tables;        // [n_motifs][m][8] device
    const int64_t *rec_off, *rec_len;   // [n_rec]
    const int64_t *tile_start;   // [n_rec + 1] prefix of ceil(L / MO_TILE)
    int64_t n_rec, n_pos;
    const double *occ;           // [n_rec][n_motifs]: events
    int m, n_motifs;
    double *local;               // dense: [n_motifs][n_pos][4]
    double frac;                 // events
    int64_t capacity;
    int64_t *ev_key;             // [capacity] (q * n_pos + p) * 4 + a
    double *ev_alt, *ev_ref;     // [capacity] local[p][a], local[p][c_p]
    unsigned long long *ev_count;
};

// the events of a tile under one motif wait here and leave with one returning atomic; a position has at most 3
struct MoQueue {
    unsigned long long base;     // the workgroup's first slot, thread 0 -> everybody
    double alt[3 * MO_TILE];
    double ref[MO_TILE];         // by position: written where the position has an event
    uint16_t key[3 * MO_TILE];   // 4 * (position - the tile's first) + letter
    int n;
};
struct MoNoQueue {};

// what the tile's workgroup knows before the first motif
struct MoTile {
    int64_t r, p0;               // the record; the tile's first position in the stream
    int n_tp;                    // positions of the tile, >= 1
};

// The strip of codes under the windows over the tile -> cl (byte b is position t0 - (m - 1) + b of the record; 0xFF where that
// lies outside the record or holds a code >= 4), and whether the window that begins at byte x has a term in the stream as it
// is -> hs.  Ends with a barrier.
__device__ __forceinline__ MoTile mo_stage(const MoArgs &a, uint8_t *cl, uint8_t *hs)
{
    const int t = threadIdx.x, m = a.m;
    MoTile T;
    T.r = occ_record(a.tile_start, 0, a.n_rec, (int64_t)blockIdx.x);
    const int64_t L = a.rec_len[T.r], off = a.rec_off[T.r];
    const int64_t t0 = ((int64_t)blockIdx.x - a.tile_start[T.r]) * MO_TILE;   // the tile's first position, within the record
    T.n_tp = (int)min((int64_t)MO_TILE, L - t0);
    T.p0 = off + t0;
    const int64_t w0 = t0 - (m - 1);                               // the position of strip byte 0: may be < 0
    const int n_byte = T.n_tp + 2 * (m - 1);                       // strip bytes that matter, <= MO_CS
    for (int i = t; i < MO_CS; i += BLOCK) {
        const int64_t x = w0 + i;
        uint8_t c = MO_FOREIGN;
        if (i < n_byte && x >= 0 && x < L) {                       // inside the record: inside the stream
            c = a.codes[off + x] & 7u;
            if (c >= 4) c = MO_FOREIGN;
        }
        cl[i] = c;
    }
    __syncthreads();
    for (int x = t; x < MO_SLOTS; x += BLOCK) {                    // x + m - 1 <= MO_SLOTS - 1 + MO_HALO < MO_CS
        bool h = x < T.n_tp + m - 1;
        if (h)
            for (int k = 0; k < m; ++k) h = h && cl[x + k] != MO_FOREIGN;
        hs[x] = h ? 1 : 0;
    }
    __syncthreads();
    return T;
}

// bit j: the window that begins j before position i of the tile (strip byte i + m - 1 - j) has a term
__device__ __forceinline__ uint64_t mo_has(const uint8_t *hs, int i, int m)
{
    uint64_t h = 0;
    for (int j = 0; j < m; ++j) h |= (uint64_t)hs[i + m - 1 - j] << j;
    return h;
}

// what a position reports: the dense row, or its events
template <bool EVENTS, typename Q>
__device__ __forceinline__ void mo_report(const MoArgs &a, Q &qu, const MoTile &T, int q, int i, int c, double lim, double l0, double l1, double l2,
                                          double l3)
{
    if constexpr (EVENTS) {
        // a position without a letter (four NaN in the dense form) compares like any other and is masked afterwards
        const double ref = c == 0 ? l0 : c == 1 ? l1 : c == 2 ? l2 : l3;
        const double d0 = l0 - ref, d1 = l1 - ref, d2 = l2 - ref, d3 = l3 - ref;
        const double nlim = -lim;
        uint32_t mask = ((d0 > lim || d0 < nlim) ? 1u : 0u) | ((d1 > lim || d1 < nlim) ? 2u : 0u) | ((d2 > lim || d2 < nlim) ? 4u : 0u) |
                        ((d3 > lim || d3 < nlim) ? 8u : 0u);       // strict: NaN never passes
        mask = c < 4 ? mask & ~(1u << c) : 0u;
        if (mask) {
            int z = atomicAdd(&qu.n, __popc(mask));                // LDS; at most 3 * n_tp per motif
            qu.ref[i] = ref;
            const double alt[4] = {l0, l1, l2, l3};
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (mask & (1u << b)) {
                    qu.key[z] = (uint16_t)(4 * i + b);
                    qu.alt[z] = alt[b];
                    ++z;
                }
        }
    } else {
        if (c >= 4) l0 = l1 = l2 = l3 = __builtin_nan("");
        f64x2 *dst = reinterpret_cast<f64x2 *>(a.local + ((int64_t)q * a.n_pos + T.p0 + i) * 4);
        dst[0] = f64x2{l0, l1};
        dst[1] = f64x2{l2, l3};
    }
}

// the tile's events under motif q -> the caller's arrays (slots at or beyond the capacity are counted, never stored); all threads
__device__ __forceinline__ void mo_flush(const MoArgs &a, MoQueue &qu, const MoTile &T, int q)
{
    __syncthreads();
    const int n = qu.n;
    if (n == 0) return;                                            // uniform: read behind the barrier
    const HitShard shard{a.ev_count, 1, a.capacity};
    if (threadIdx.x == 0) qu.base = shard.reserve((unsigned long long)n);
    __syncthreads();
    const unsigned long long base = qu.base;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const unsigned long long slot = base + (unsigned long long)i;
        if (shard.in_range(slot)) {
            const int k = qu.key[i];
            a.ev_key[slot] = ((int64_t)q * a.n_pos + T.p0 + (k >> 2)) * 4 + (k & 3);
            a.ev_alt[slot] = qu.alt[i];
            a.ev_ref[slot] = qu.ref[k >> 2];
        }
    }
}

// the head of a motif's round: the table -> LDS, the queue emptied; ends with a barrier
template <bool EVENTS, typename Q> __device__ __forceinline__ void mo_motif(const MoArgs &a, double *tab, Q &qu, int q)
{
    if (q != 0) __syncthreads();                                   // the readers of the last motif's table and queue are done
    for (int i = threadIdx.x; i < a.m * 8; i += BLOCK) tab[i] = a.tables[(int64_t)q * a.m * 8 + i];
    if constexpr (EVENTS)
        if (threadIdx.x == 0) qu.n = 0;
    __syncthreads();
}

// The empty asm behind every window ties the four sums to a point in the order of the volatile table reads.  Without it hipcc
// schedules the EVENTS form -- whose sums end in compares and a branch, not in stores -- with all M (M - 1) table reads of a
// position in front of the first product: 137 VGPRs at M = 8, 290 at 12, spills at 20, and the events form ran 8.1 / 26.0 ms
// at w = 8 / 12 where the dense form ran 5.9 / 9.0 (profiles/mutocc/NOTES.md).  __builtin_amdgcn_sched_barrier did not change
// that; the asm does: 53 .. 78 VGPRs in both forms.
template <int M, bool EVENTS>
__global__ __launch_bounds__(BLOCK) void k_mutocc(const MoArgs a)
{
    static_assert(M >= 1 && M <= MO_FIXED_MAX, "width outside this kernel's range");
    constexpr int NB = 2 * M - 1;                                  // codes around a position: offsets -(M - 1) .. M - 1
    __shared__ __align__(16) double tab[M * 8];
    __shared__ __align__(16) uint8_t cl[MO_CS];
    __shared__ uint8_t hs[MO_SLOTS];
    __shared__ std::conditional_t<EVENTS, MoQueue, MoNoQueue> qu;
    const MoTile T = mo_stage(a, cl, hs);

    typedef const volatile __attribute__((address_space(3))) double *lds_f64;   // one ds_read_b64 per look-up (k_mutmap)
    typedef const __attribute__((address_space(3))) char *lds_bytes;
    const lds_bytes tb = (lds_bytes)reinterpret_cast<const char *>(tab);
    for (int q = 0; q < a.n_motifs; ++q) {
        mo_motif<EVENTS>(a, tab, qu, q);
        // R[j][a] of the substituted letter: uniform addresses in the constant address space, i.e. scalar loads and operands
        const __attribute__((address_space(4))) double *R = (const __attribute__((address_space(4))) double *)(a.tables + (int64_t)q * M * 8);
        double lim = 0.0;
        if constexpr (EVENTS) lim = a.frac * a.occ[T.r * a.n_motifs + q];
#pragma unroll 1
        for (int g = 0; g < MO_PPL; ++g) {
            const int i = (int)threadIdx.x + g * BLOCK;
            if (i >= T.n_tp) continue;
            const uint8_t *nbp = cl + i;                           // byte i + q: offset q - (M - 1) from the position
            uint32_t adr[NB];                                      // byte offset of the code's column in a table row; foreign: column 7
            static_for<0, NB>([&](auto qc) __attribute__((always_inline)) {
                constexpr int z = decltype(qc)::value;
                adr[z] = ((uint32_t)nbp[z] & 7u) << 3;
            });
            const int c = nbp[M - 1] == MO_FOREIGN ? 7 : (int)(adr[M - 1] >> 3);
            const uint64_t hm = mo_has(hs, i, M);                  // m byte reads against 2.5 m^2 products
            double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
            static_for<0, M>([&](auto jc) __attribute__((always_inline)) {
                constexpr int j = M - 1 - decltype(jc)::value;     // the lowest start first; window letter k is adr[M - 1 - j + k]
                double x0 = R[j * 8 + 0], x1 = R[j * 8 + 1], x2 = R[j * 8 + 2], x3 = R[j * 8 + 3];
                if constexpr (j > 0) {
                    double pre = *(lds_f64)(tb + adr[M - 1 - j]);
                    static_for<1, j>([&](auto kc) __attribute__((always_inline)) {
                        constexpr int k = decltype(kc)::value;
                        pre = pre * *(lds_f64)(tb + k * 64 + adr[M - 1 - j + k]);
                    });
                    x0 = pre * x0;
                    x1 = pre * x1;
                    x2 = pre * x2;
                    x3 = pre * x3;
                }
                static_for<j + 1, M>([&](auto kc) __attribute__((always_inline)) {
                    constexpr int k = decltype(kc)::value;
                    const double f = *(lds_f64)(tb + k * 64 + adr[M - 1 - j + k]);
                    x0 = x0 * f;
                    x1 = x1 * f;
                    x2 = x2 * f;
                    x3 = x3 * f;
                });
                const bool ok = (hm >> j) & 1u;                    // without a term the window adds +0.0
                l0 = l0 + (ok ? x0 : 0.0);
                l1 = l1 + (ok ? x1 : 0.0);
                l2 = l2 + (ok ? x2 : 0.0);
                l3 = l3 + (ok ? x3 : 0.0);
                asm volatile("" : "+v"(l0), "+v"(l1), "+v"(l2), "+v"(l3));   // a window at a time: see above the kernel
            });
            mo_report<EVENTS>(a, qu, T, q, i, c, lim, l0, l1, l2, l3);
        }
        if constexpr (EVENTS) mo_flush(a, qu, T, q);
    }
}

template <bool EVENTS>
__global__ __launch_bounds__(BLOCK) void k_mutocc_rolled(const MoArgs a)
{
    __shared__ __align__(16) double tab[PFMSCAN_MAX_M * 8];
    __shared__ __align__(16) uint8_t cl[MO_CS];
    __shared__ uint8_t hs[MO_SLOTS];
    __shared__ std::conditional_t<EVENTS, MoQueue, MoNoQueue> qu;
    const int m = a.m;
    const MoTile T = mo_stage(a, cl, hs);
    for (int q = 0; q < a.n_motifs; ++q) {
        mo_motif<EVENTS>(a, tab, qu, q);
        const __attribute__((address_space(4))) double *R = (const __attribute__((address_space(4))) double *)(a.tables + (int64_t)q * m * 8);
        double lim = 0.0;
        if constexpr (EVENTS) lim = a.frac * a.occ[T.r * a.n_motifs + q];
#pragma unroll 1
        for (int g = 0; g < MO_PPL; ++g) {
            const int i = (int)threadIdx.x + g * BLOCK;
            if (i >= T.n_tp) continue;
            const uint8_t *here = cl + i + (m - 1);
            const int c = here[0] == MO_FOREIGN ? 7 : (int)here[0];
            double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
#pragma unroll 1
            for (int j = m - 1; j >= 0; --j) {
                const uint8_t *w = here - j;                       // the window's first letter: >= cl
                double x0 = R[j * 8 + 0], x1 = R[j * 8 + 1], x2 = R[j * 8 + 2], x3 = R[j * 8 + 3];
                if (j > 0) {
                    double pre = tab[w[0] & 7];
#pragma unroll 1
                    for (int k = 1; k < j; ++k) pre = pre * tab[k * 8 + (w[k] & 7)];
                    x0 = pre * x0;
                    x1 = pre * x1;
                    x2 = pre * x2;
                    x3 = pre * x3;
                }
#pragma unroll 1
                for (int k = j + 1; k < m; ++k) {
                    const double f = tab[k * 8 + (w[k] & 7)];
                    x0 = x0 * f;
                    x1 = x1 * f;
                    x2 = x2 * f;
                    x3 = x3 * f;
                }
                const bool ok = hs[i + m - 1 - j] != 0;
                l0 = l0 + (ok ? x0 : 0.0);
                l1 = l1 + (ok ? x1 : 0.0);
                l2 = l2 + (ok ? x2 : 0.0);
                l3 = l3 + (ok ? x3 : 0.0);
            }
            mo_report<EVENTS>(a, qu, T, q, i, c, lim, l0, l1, l2, l3);
        }
        if constexpr (EVENTS) mo_flush(a, qu, T, q);
    }
}

template <bool EVENTS> static hipError_t launch_mutocc(const MoArgs &a, unsigned grid, hipStream_t st)
{
    const bool rolled = std::getenv("PFMSCAN_MUTOCC_ROLLED") != nullptr;   // tests and A/B runs: the rolled kernel at every width
    switch (rolled ? 0 : a.m) {
#define MO_WIDTH(W) case W: hipLaunchKernelGGL((k_mutocc<W, EVENTS>), dim3(grid), dim3(BLOCK), 0, st, a); break;
    MO_WIDTH(1) MO_WIDTH(2) MO_WIDTH(3) MO_WIDTH(4) MO_WIDTH(5) MO_WIDTH(6) MO_WIDTH(7) MO_WIDTH(8) MO_WIDTH(9) MO_WIDTH(10)
    MO_WIDTH(11) MO_WIDTH(12) MO_WIDTH(13) MO_WIDTH(14) MO_WIDTH(15) MO_WIDTH(16) MO_WIDTH(17) MO_WIDTH(18) MO_WIDTH(19) MO_WIDTH(20)
#undef MO_WIDTH
    default: hipLaunchKernelGGL((k_mutocc_rolled<EVENTS>), dim3(grid), dim3(BLOCK), 0, st, a); break;
    }
    return hipGetLastError();
}

// Launches on st, does not wait.  The FpOut of the posterior site map carries what a call leaves: `cover` is the dense map
// local, thr is frac, ev_cover the alt value of an event and ev_start its ref value.
static int mo_run(pfmscan_ctx *ctx, const char *who, const double *seq_tables, int n_motifs, int m, const uint8_t *d_codes, const OccRecords &rec,
                  const FpOut &o, double *d_occ, int64_t *d_windows, hipStream_t st)
{
    int rc;
    const int64_t pairs = rec.n_rec * n_motifs;
    // the occupancy of the same records first: what the events compare with, and what the caller asked for
    if (o.events || d_occ || d_windows) {
        if (!d_occ) {
            if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
            d_occ = (double *)ctx->exp_occ.p;
        }
        if ((rc = occ_run(ctx, who, seq_tables, n_motifs, m, 4, d_codes, rec, d_occ, d_windows, st))) return rc;
    }
    std::vector<int64_t> tiles;
    const int64_t n_tiles = fp_tile_prefix(rec.len, rec.n_rec, MO_TILE, tiles);
    if (n_tiles == 0) return PFMSCAN_OK;
    if (n_tiles < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many positions for one call");
    if ((rc = ensure(ctx, ctx->fp_idx, tiles.size() * 8))) return rc;
    if ((rc = upload(ctx, ctx->fp_idx.p, tiles.data(), tiles.size() * 8, st))) return rc;
    MoArgs a{};
    const double *none = nullptr;
    if ((rc = occ_upload_tables(ctx, seq_tables, nullptr, 0, n_motifs, m, st, a.tables, none))) return rc;
    a.codes = d_codes;
    a.rec_off = rec.d_off;
    a.rec_len = rec.d_len;
    a.tile_start = (const int64_t *)ctx->fp_idx.p;
    a.n_rec = rec.n_rec;
    a.n_pos = rec.n_pos;
    a.occ = d_occ;
    a.m = m;
    a.n_motifs = n_motifs;
    a.local = o.cover;
    a.frac = o.thr;
    a.capacity = o.capacity;
    a.ev_key = o.ev_key;
    a.ev_alt = o.ev_cover;
    a.ev_ref = o.ev_start;
    a.ev_count = o.ev_count;
    const hipError_t e = o.events ? launch_mutocc<true>(a, (unsigned)n_tiles, st) : launch_mutocc<false>(a, (unsigned)n_tiles, st);
    return e != hipSuccess ? fail_hip(ctx, e, "k_mutocc") : PFMSCAN_OK;
}

// the checks of all four entry points up to "n_rec == 0 or n_motifs == 0: nothing to do"
static int mo_check(pfmscan_ctx *ctx, const char *who, const double *seq_tables, int n_motifs, int m, int64_t n_pos, int64_t n_rec)
{
    return occ_check_base(ctx, who, m, nullptr, n_motifs, n_rec, n_pos, seq_tables ? nullptr : ": seq_tables is NULL");
}

static int mo_check_events(pfmscan_ctx *ctx, const char *who, double frac, int64_t capacity, const void *count, const void *key, const void *alt,
                           const void *ref)
{
    if (std::isnan(frac) || frac < 0.0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": frac is negative or not a number");
    return fp_check_events(ctx, who, frac, capacity, count, key, alt, ref);
}

// both _dev forms
static int mo_dev(pfmscan_ctx *ctx, const char *who, const double *seq_tables, int n_motifs, int m, const uint8_t *d_codes, int64_t n_pos,
                  const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, const FpOut &o, double *d_occ, int64_t *d_windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = mo_check(ctx, who, seq_tables, n_motifs, m, n_pos, n_rec)) return rc;
    if (o.events) {
        if (int rc = mo_check_events(ctx, who, o.thr, o.capacity, o.ev_count, o.ev_key, o.ev_cover, o.ev_start)) return rc;
    } else if (!o.cover) {
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": d_local is NULL");
    }
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!d_rec_off || !d_rec_len || (n_pos > 0 && !d_codes)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table or codes");
    if (misaligned(d_codes)) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    if (misaligned(o.cover)) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": d_local must be 16-byte aligned");
    std::vector<int64_t> host;
    OccRecords rec;
    if (int rc = occ_records_home(ctx, who, d_rec_off, d_rec_len, n_rec, n_pos, host, rec)) return rc;
    return mo_run(ctx, who, seq_tables, n_motifs, m, d_codes, rec, o, d_occ, d_windows, ctx->stream);
}

static int mo_staged_check(pfmscan_ctx *ctx, const char *who)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes are staged");
    return PFMSCAN_OK;
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_mutocc_dev(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const uint8_t *d_codes, int64_t n_pos,
                       const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double *d_local, double *d_occ, int64_t *d_windows)
{
    const FpOut o{nullptr, d_local, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    return mo_dev(ctx, "pfmscan_mutocc_dev", seq_tables, n_motifs, m, d_codes, n_pos, d_rec_off, d_rec_len, n_rec, o, d_occ, d_windows);
}

int pfmscan_mutocc_events_dev(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const uint8_t *d_codes, int64_t n_pos,
                              const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec, double frac, int64_t capacity, int64_t *d_ev_key,
                              double *d_ev_alt, double *d_ev_ref, uint64_t *d_ev_count, double *d_occ, int64_t *d_windows)
{
    const FpOut o{nullptr, nullptr, true, frac, capacity, d_ev_key, d_ev_alt, d_ev_ref, reinterpret_cast<unsigned long long *>(d_ev_count)};
    return mo_dev(ctx, "pfmscan_mutocc_events_dev", seq_tables, n_motifs, m, d_codes, n_pos, d_rec_off, d_rec_len, n_rec, o, d_occ, d_windows);
}

int pfmscan_mutocc_staged(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const int64_t *rec_off, const int64_t *rec_len,
                          int64_t n_rec, double *local, double *occ, int64_t *windows)
{
    const char *who = "pfmscan_mutocc_staged";
    if (int rc = mo_staged_check(ctx, who)) return rc;
    const int64_t n_pos = ctx->staged_n;
    if (int rc = mo_check(ctx, who, seq_tables, n_motifs, m, n_pos, n_rec)) return rc;
    if (!local) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": local is NULL");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const size_t plane = (size_t)n_motifs * (size_t)n_pos * 4, pairs = (size_t)n_rec * n_motifs;
    if ((rc = ensure(ctx, ctx->fp_out, std::max<size_t>((plane + pairs + (size_t)n_rec) * 8, 16)))) return rc;
    double *d_local = (double *)ctx->fp_out.p;
    double *d_occ = occ ? d_local + plane : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_local + plane + pairs) : nullptr;
    // positions in no record of the table are NaN: every byte 0xFF is one
    if (plane) HIP_TRY(ctx, hipMemsetAsync(d_local, 0xFF, plane * 8, ctx->stream));
    const FpOut o{nullptr, d_local, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    if ((rc = mo_run(ctx, who, seq_tables, n_motifs, m, (const uint8_t *)ctx->codes.p, rec, o, d_occ, d_win, ctx->stream))) return rc;
    return occ_copy_home(ctx, {{local, d_local, plane * 8}, {occ, d_occ, pairs * 8}, {windows, d_win, (size_t)n_rec * 8}});
}

int pfmscan_mutocc_events_staged(pfmscan_ctx *ctx, const double *seq_tables, int n_motifs, int m, const int64_t *rec_off, const int64_t *rec_len,
                                 int64_t n_rec, double frac, int64_t capacity, int64_t *ev_key, double *ev_alt, double *ev_ref, int64_t *n_events,
                                 double *occ, int64_t *windows)
{
    const char *who = "pfmscan_mutocc_events_staged";
    if (int rc = mo_staged_check(ctx, who)) return rc;
    const int64_t n_pos = ctx->staged_n;
    if (int rc = mo_check(ctx, who, seq_tables, n_motifs, m, n_pos, n_rec)) return rc;
    if (int rc = mo_check_events(ctx, who, frac, capacity, n_events, ev_key, ev_alt, ev_ref)) return rc;
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
    if ((rc = fp_events_room(ctx, frac, capacity, pairs, (size_t)n_rec, occ != nullptr, windows != nullptr, o, d_occ, d_win))) return rc;
    if ((rc = mo_run(ctx, who, seq_tables, n_motifs, m, (const uint8_t *)ctx->codes.p, rec, o, d_occ, d_win, ctx->stream))) return rc;
    return fp_events_home(ctx, who, o, ev_key, ev_alt, ev_ref, n_events, {occ, d_occ, pairs * 8}, {windows, d_win, (size_t)n_rec * 8});
}

}  // extern "C"
