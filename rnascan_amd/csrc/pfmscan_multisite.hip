// pfmscan_multisite.hip -- the multi-site model: the partition function over all sets of non-overlapping sites of a record
// and its forward-backward site posteriors (include/pfmscan.h "multi-site model").
//
// The activity of window s is a_s = t_s * lam_r, t_s the family's term.  F[i] = F[i-1] + a[i-m] F[i-m] walks the record
// forward, B[i] = B[i+1] + a[i] B[i+m] backward, Z = F[L], and the posterior that a site starts at s is
// ((F[s] a[s]) B[s+m]) / Z.  Every operation is one rounded fp64 product or addition in a fixed order: no transcendental, no
// atomics on doubles, no tolerance; tests/multisite_rules.py restates it in numpy and the bits are compared.
//
// Four kernels per pass (a pass: the records and motifs whose two scratch planes fit the cap, pfmscan_ms_plan.hpp):
//   k_ms_terms     tile-parallel, the geometry of k_fp_tiles: a workgroup owns a tile of ONE record, parks the strip(s) of codes
//                  in LDS, and a lane makes the chain of its windows and stores a_s into plane A.  Everything with m in it.
//   k_ms_profile_terms<T, SEQ>
//                  takes k_ms_terms' place when the stream is an averaged-structure profile (DESIGN.md 5n "on averaged-structure
//                  profiles"): the same tile of ONE record, the rows under its windows fetched as aligned 16-byte vectors
//                  (occp_load), clipped to the record and parked in LDS as doubles, the chain of k_fp_profile_tiles
//                  (occp_marginal per row, in joint mode behind the letter chain), a_s into plane A.  No halo: rows
//                  [t0, min(t0 + n_tp + m - 1, L)) only.
//   k_ms_forward   ONE LANE per (record, motif), a wave per workgroup.  The wave moves MS_CHUNK activities of each of its 64
//                  records through LDS at a time (a run of consecutive doubles per record, never 8-byte accesses a record
//                  apart; the next chunk's loads are in flight in registers meanwhile), every lane then walks its own row: g = a[j] * F[j] does not depend on F[j+m-1], only the
//                  addition F[j+m] = F[j+m-1] + g is on the critical path.  The last m values of F wait in an LDS ring
//                  ring[slot][lane] (no register is indexed at run time).  g replaces a in the chunk and leaves for plane G:
//                  the backward walk needs the product F[s] a[s], not F itself (products commute bit for bit).  Z leaves last.
//   k_ms_backward  the same walk descending: a ring of B (never stored), reads A and G, start[s] = (g_s * B[s+m]) * v replaces g
//                  in plane G, nsites is added up on the way (descending, as the contract says).
//   k_ms_cover     tile-parallel: the adder and the event queue of k_fp_tiles over plane G.
// Lanes of a wave have records of unequal length: the trip count of the chunk loop is the wave's longest, a lane that is done
// takes part in the barriers and the loads of the others and computes nothing.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_device.hpp"
#include "pfmscan_fp.hpp"
#include "pfmscan_fp_plan.hpp"
#include "pfmscan_ms_plan.hpp"
#include "pfmscan_occ.hpp"

#pragma clang fp contract(off)   // products and sums are rounded one operation at a time: never an FMA

namespace pfmscan {

constexpr int MS_SLOTS = PFMSCAN_MULTISITE_SLOTS;                  // windows of a workgroup of the tile-parallel kernels
constexpr int MS_WPL = MS_SLOTS / BLOCK;                           // windows (and positions) of a lane
constexpr int MS_CS = (MS_SLOTS + PFMSCAN_MAX_M - 1 + 3) / 4 * 4;  // bytes of a strip of codes
constexpr uint8_t MS_FOREIGN = 0xFF;
constexpr int MSP_ROWS = MS_SLOTS + PFMSCAN_MAX_M - 1;             // profile rows under the windows of a tile, at most
constexpr int MS_CHUNK = PFMSCAN_MULTISITE_CHUNK;                  // positions of a record a serial kernel holds in LDS
constexpr int MS_ROW = MS_CHUNK + 1;                               // doubles of a lane's row: odd, so that a wave's rows fall on distinct banks
constexpr int MS_LANES = 64;                                       // (record, motif) pairs of a workgroup of the serial kernels: one wave
constexpr int64_t MS_SCRATCH_DOUBLES = int64_t(1) << 28;           // both planes of one pass (2 GiB); PFMSCAN_MULTISITE_SCRATCH_DOUBLES overrides
static_assert(MS_WPL * BLOCK == MS_SLOTS && MS_SLOTS > PFMSCAN_MAX_M - 1 && MS_SLOTS <= 65536, "whole lanes, a tile of at least one position, 16-bit queue");
static_assert((MS_ROW & 1) == 1, "an odd row stride");
// the backward kernel: two chunks, the ring at the widest motif and the lane tables stay inside 64 KB of LDS
static_assert(2 * MS_LANES * MS_ROW * 8 + MS_LANES * PFMSCAN_MAX_M * 8 + MS_LANES * 16 <= 65536, "LDS of k_ms_backward");

struct MsArgs {
    const uint8_t *codes;        // [n_pos] the first strip: RNA codes, or the structure-letter codes of a structure-only call
    const uint8_t *codes2;       // [n_pos] PAIR: structure-letter codes
    const double *tables;        // [n_motifs][m][8] device: the tables over codes
    const double *tables2;       // PAIR: the structure tables
    const unsigned char *profile;   // [n_pos][7] float or double, 16-byte aligned, or null: an averaged-structure profile takes the
                                 // place of the strips; then tables are the letter tables of joint mode over codes (or null) and
                                 // tables2 the structure tables [n_motifs][m][7] in the profile's stored column order
    int dtype;                   // PFMSCAN_PROFILE_F32 / F64
    bool joint;                  // profile: the letter chain first, a window with a code >= 4 has no term
    const int64_t *rec_off, *rec_len;   // [n_rec]
    const int64_t *tile_start;   // [n_rec + 1] prefix of ceil(L / tile)
    const double *lam;           // [n_rec] device
    int64_t n_pos;
    int64_t r0, r1;              // records of this pass
    int64_t tile_base;           // tile_start[r0]
    int64_t base, span;          // stream position p lies at p - base of a scratch plane of span doubles
    int q0, nq;                  // motifs of this pass
    int n_motifs, m, nl, tile;
    double *pa, *pg;             // [nq][span] scratch: the activities; the forward products, then the site posteriors
    double *z;                   // [n_rec][n_motifs], never null
    double *nsites;              // [n_rec][n_motifs] or null
    unsigned long long *windows; // [n_rec] zeroed, or null: only the pass of motif 0 counts
    double *start, *cover;       // [n_motifs][n_pos], either may be null (maps)
    double thr;                  // events
    int64_t capacity;
    int64_t *ev_key;
    double *ev_cover, *ev_start;
    unsigned long long *ev_count;
};

// ---- (a) the activities -------------------------------------------------------------------------------------------------
template <bool PAIR>
__global__ __launch_bounds__(BLOCK) void k_ms_terms(const MsArgs a)
{
    constexpr int NS = PAIR ? 2 : 1;
    __shared__ double tab[NS][PFMSCAN_MAX_M * 8];
    __shared__ uint8_t cl[NS][MS_CS];
    const int t = threadIdx.x, m = a.m;
    const int64_t r = occ_record(a.tile_start, a.r0, a.r1, a.tile_base + (int64_t)blockIdx.x);
    const int64_t L = a.rec_len[r], off = a.rec_off[r];
    const int64_t t0 = (a.tile_base + (int64_t)blockIdx.x - a.tile_start[r]) * a.tile;   // the tile's first position, within the record
    const int n_tp = (int)min((int64_t)a.tile, L - t0);            // its positions, >= 1: the tile exists
    const int n_byte = n_tp + m - 1;                               // strip bytes under its windows, <= MS_CS
    for (int i = t; i < MS_CS; i += BLOCK) {
        const int64_t x = t0 + i;
        uint8_t c0 = MS_FOREIGN, c1 = MS_FOREIGN;
        if (i < n_byte && x < L) {                                 // inside the record: inside the stream
            c0 = a.codes[off + x] & 7u;
            if ((int)c0 >= a.nl) c0 = MS_FOREIGN;
            if constexpr (PAIR) {
                c1 = a.codes2[off + x] & 7u;
                if ((int)c1 >= PFMSCAN_NSTRUCT) c1 = MS_FOREIGN;
            }
        }
        cl[0][i] = c0;
        if constexpr (PAIR) cl[1][i] = c1;
    }
    __syncthreads();
    const int64_t n_win = L - m + 1;                               // may be <= 0: then no slot is a window
    bool has[MS_WPL], win[MS_WPL];
#pragma unroll
    for (int j = 0; j < MS_WPL; ++j) {
        const int s = t + j * BLOCK;
        win[j] = s < n_tp && t0 + s < n_win;
        bool h = win[j];
        if (h)
            for (int k = 0; k < m; ++k) {
                h = h && cl[0][s + k] != MS_FOREIGN;
                if constexpr (PAIR) h = h && cl[1][s + k] != MS_FOREIGN;
            }
        has[j] = h;
    }
    if (a.windows) {                                               // uniform
        int n = 0;
#pragma unroll
        for (int j = 0; j < MS_WPL; ++j) n += __syncthreads_count(has[j]);
        if (t == 0 && n != 0) atomicAdd(&a.windows[r], (unsigned long long)n);   // integers: the order does not matter
    }
    const double lam = a.lam[r];
    const int64_t p0 = off - a.base + t0;                          // the tile's first position, in a plane
    for (int q = 0; q < a.nq; ++q) {
        if (q != 0) __syncthreads();                               // the chains of the last motif are done with the tables
        for (int i = t; i < m * 8; i += BLOCK) {
            tab[0][i] = a.tables[(int64_t)(a.q0 + q) * m * 8 + i];
            if constexpr (PAIR) tab[1][i] = a.tables2[(int64_t)(a.q0 + q) * m * 8 + i];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MS_WPL; ++j) {
            const int s = t + j * BLOCK;
            if (s < n_tp) {
                double act = 0.0;                                  // a position that starts no window
                if (win[j]) {
                    double x = 0.0;                                // a window without a term
                    if (has[j]) {
                        const uint8_t *cp = &cl[0][s];
                        x = tab[0][cp[0]];
                        for (int k = 1; k < m; ++k) x = x * tab[0][k * 8 + cp[k]];
                        if constexpr (PAIR) {
                            cp = &cl[1][s];
                            for (int k = 0; k < m; ++k) x = x * tab[1][k * 8 + cp[k]];
                        }
                    }
                    act = x * lam;
                }
                a.pa[(int64_t)q * a.span + p0 + s] = act;
            }
        }
    }
}

// ---- (a') the activities of an averaged-structure profile ---------------------------------------------------------------
// The tables, the profile and the plane are separate __restrict__ arguments: the table rows are workgroup-uniform and stay
// scalar operands while plane A is stored.
template <typename T, bool SEQ>
__global__ __launch_bounds__(BLOCK) void k_ms_profile_terms(const MsArgs a, const unsigned char *__restrict__ profile, const uint8_t *__restrict__ codes,
                                                            const double *__restrict__ stab, const double *__restrict__ ltab,
                                                            double *__restrict__ pa)
{
    constexpr int RB = 7 * (int)sizeof(T);                         // bytes of a row
    constexpr int PER = 16 / (int)sizeof(T);                       // cells of a vector
    __shared__ double rows[MSP_ROWS * 7];
    __shared__ uint8_t cl[SEQ ? MS_CS : 8];
    const int t = threadIdx.x, m = a.m;
    const int64_t r = occ_record(a.tile_start, a.r0, a.r1, a.tile_base + (int64_t)blockIdx.x);
    const int64_t L = a.rec_len[r], off = a.rec_off[r];
    const int64_t t0 = (a.tile_base + (int64_t)blockIdx.x - a.tile_start[r]) * a.tile;   // the tile's first position, within the record
    const int n_tp = (int)min((int64_t)a.tile, L - t0);            // its positions, >= 1: the tile exists
    const int64_t n_win = L - m + 1;                               // may be <= 0: then no slot is a window
    {
        // the rows of the record under the tile's windows: [t0, hi), clipped to the record's end; row x lies at LDS row x - t0
        const int64_t hi = min(t0 + n_tp + m - 1, L);
        const int nrows = (int)(hi - t0);                          // 1 .. MSP_ROWS
        const int64_t first = (off + t0) * RB, end = first + (int64_t)nrows * RB, base = first & ~(int64_t)15, total = a.n_pos * RB;
        const int shift = (int)(first - base) / (int)sizeof(T);
        const int ncell = nrows * 7, nvec = (int)((end - base + 15) / 16);
        for (int v = t; v < nvec; v += BLOCK) {
            double d[PER];
            occp_cells(occp_load(profile, base + (int64_t)v * 16, total), d, T());
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int idx = v * PER + j - shift;
                if (idx >= 0 && idx < ncell) rows[idx] = d[j];
            }
        }
        if constexpr (SEQ)
            for (int i = t; i < MS_CS; i += BLOCK) {
                const int64_t x = t0 + i;
                uint8_t c = MS_FOREIGN;
                if (i < n_tp + m - 1 && x < L) {                   // inside the record: inside the stream
                    c = codes[off + x] & 7u;
                    if (c >= 4u) c = MS_FOREIGN;
                }
                cl[i] = c;
            }
    }
    __syncthreads();
    // a slot is a window by 0 <= s < n_win, never by what was loaded; in joint mode it has a term when it holds no foreign code
    bool has[MS_WPL], win[MS_WPL];
#pragma unroll
    for (int j = 0; j < MS_WPL; ++j) {
        const int s = t + j * BLOCK;
        win[j] = s < n_tp && t0 + s < n_win;
        bool h = win[j];
        if constexpr (SEQ) {
            if (h)
                for (int k = 0; k < m; ++k) h = h && cl[s + k] != MS_FOREIGN;
        }
        has[j] = h;
    }
    if (a.windows) {                                               // uniform
        int n = 0;
#pragma unroll
        for (int j = 0; j < MS_WPL; ++j) n += __syncthreads_count(has[j]);
        if (t == 0 && n != 0) atomicAdd(&a.windows[r], (unsigned long long)n);   // integers: the order does not matter
    }
    const double lam = a.lam[r];
    const int64_t p0 = off - a.base + t0;                          // the tile's first position, in a plane
    const int64_t ms = (int64_t)m * 7, ml = (int64_t)m * 8;
    for (int q = 0; q < a.nq; ++q) {                               // the tables of the next motif, the rows stay
        const double *sp = stab + (a.q0 + q) * ms;
#pragma unroll
        for (int j = 0; j < MS_WPL; ++j) {
            const int s = t + j * BLOCK;
            if (s < n_tp) {
                double act = 0.0;                                  // a position that starts no window
                if (win[j]) {
                    double tt = 0.0;                               // a window without a term
                    if (has[j]) {
                        if constexpr (SEQ) {
                            const double *lt = ltab + (a.q0 + q) * ml;
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
                    }
                    act = tt * lam;
                }
                pa[(int64_t)q * a.span + p0 + s] = act;
            }
        }
    }
}

template <typename T>
static void ms_launch_profile_terms(const MsArgs &a, const dim3 grid, hipStream_t st)
{
    if (a.joint) hipLaunchKernelGGL((k_ms_profile_terms<T, true>), grid, dim3(BLOCK), 0, st, a, a.profile, a.codes, a.tables2, a.tables, a.pa);
    else hipLaunchKernelGGL((k_ms_profile_terms<T, false>), grid, dim3(BLOCK), 0, st, a, a.profile, a.codes, a.tables2, a.tables, a.pa);
}

// the one part of a pass that depends on what the stream is: plane A from two strips of codes, one, or profile rows
static void ms_launch_terms(const MsArgs &a, const dim3 grid, hipStream_t st)
{
    if (a.profile) {
        if (a.dtype == PFMSCAN_PROFILE_F64) ms_launch_profile_terms<double>(a, grid, st);
        else ms_launch_profile_terms<float>(a, grid, st);
    } else if (a.codes2) {
        hipLaunchKernelGGL((k_ms_terms<true>), grid, dim3(BLOCK), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_ms_terms<false>), grid, dim3(BLOCK), 0, st, a);
    }
}

// ---- (b), (c) the two walks --------------------------------------------------------------------------------------------
// what a wave of a serial kernel knows of its 64 lanes
struct MsLanes {
    int64_t at[MS_LANES];        // where the lane's record begins in its motif's plane
    int64_t nw[MS_LANES];        // its windows, 0 for a lane without a pair
};

// lane -> its pair (record r, motif q of the pass); false: the lane has none
__device__ __forceinline__ bool ms_lane(const MsArgs &a, int64_t &r, int &q)
{
    const int64_t n_r = a.r1 - a.r0, g = (int64_t)blockIdx.x * MS_LANES + threadIdx.x;
    if (g >= n_r * a.nq) return false;
    q = (int)(g / n_r);
    r = a.r0 + g % n_r;
    return true;
}

// the lanes' table, and the chunks of the wave's longest record
__device__ __forceinline__ int64_t ms_lanes_setup(const MsArgs &a, MsLanes &ln, bool ok, int64_t r, int q, int64_t &n_win)
{
    const int t = threadIdx.x;
    n_win = 0;
    int64_t at = 0;
    if (ok) {
        n_win = max(a.rec_len[r] - a.m + 1, (int64_t)0);
        at = (int64_t)q * a.span + a.rec_off[r] - a.base;
    }
    ln.at[t] = at;
    ln.nw[t] = n_win;
    __syncthreads();
    int64_t longest = 0;
    for (int i = 0; i < MS_LANES; ++i) longest = max(longest, ln.nw[i]);
    return (longest + MS_CHUNK - 1) / MS_CHUNK;
}

// Chunk k of every lane's record moves between a plane and the LDS rows as the 64 x MS_CHUNK block whose element
// e = i * 64 + t lane t takes: the lanes of the wave touch runs of consecutive doubles of a few records.  A chunk comes in two
// steps -- ms_fetch issues all MS_CHUNK loads into registers (constant indices) before anything waits for one, ms_park writes
// them to the rows -- so that the loads of the NEXT chunk are in flight while this one is walked.  With a load and its LDS
// store in one loop every load waited for the one before it (the store may alias the lane table it reads next): 14 us a chunk.
__device__ __forceinline__ void ms_fetch(const double *__restrict__ plane, const MsLanes &ln, int64_t k, double (&v)[MS_CHUNK])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < MS_CHUNK; ++i) {
        const int e = i * MS_LANES + t, row = e / MS_CHUNK, col = e % MS_CHUNK;
        const int64_t j = k * MS_CHUNK + col;
        v[i] = 0.0;
        if (j < ln.nw[row]) v[i] = plane[ln.at[row] + j];
    }
}

__device__ __forceinline__ void ms_park(double (*rows)[MS_ROW], const double (&v)[MS_CHUNK])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < MS_CHUNK; ++i) {
        const int e = i * MS_LANES + t;
        rows[e / MS_CHUNK][e % MS_CHUNK] = v[i];
    }
}

__device__ __forceinline__ void ms_flush(double *__restrict__ plane, double (*rows)[MS_ROW], const MsLanes &ln, int64_t k)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < MS_CHUNK; ++i) {
        const int e = i * MS_LANES + t, row = e / MS_CHUNK, col = e % MS_CHUNK;
        const int64_t j = k * MS_CHUNK + col;
        if (j < ln.nw[row]) plane[ln.at[row] + j] = rows[row][col];
    }
}

__global__ __launch_bounds__(MS_LANES) void k_ms_forward(const MsArgs a)
{
    __shared__ double ch[MS_LANES][MS_ROW];
    __shared__ MsLanes ln;
    extern __shared__ double ring[];                               // [m][64]: F[j] .. F[j + m - 1] of every lane
    const int t = threadIdx.x, m = a.m;
    int64_t r = 0, n_win;
    int q = 0;
    const bool ok = ms_lane(a, r, q);
    const int64_t n_chunk = ms_lanes_setup(a, ln, ok, r, q, n_win);
    for (int s = 0; s < m; ++s) ring[s * MS_LANES + t] = 1.0;      // F[0] .. F[m - 1]: 1.0 + (+0.0) each
    double f = 1.0;                                                // F[j + m - 1]
    int slot = 0;
    double va[MS_CHUNK];
    if (n_chunk > 0) ms_fetch(a.pa, ln, 0, va);
    for (int64_t k = 0; k < n_chunk; ++k) {
        ms_park(ch, va);
        __syncthreads();
        if (k + 1 < n_chunk) ms_fetch(a.pa, ln, k + 1, va);        // in flight while this chunk is walked
        const int64_t left = n_win - k * MS_CHUNK;
        const int n = (int)min((int64_t)MS_CHUNK, left);           // <= 0: this lane is done
#pragma unroll
        for (int c = 0; c < MS_CHUNK; ++c) {
            if (c < n) {
                const double g = ch[t][c] * ring[slot * MS_LANES + t];   // a[j] * F[j]
                f = f + g;                                         // F[j + m]
                ring[slot * MS_LANES + t] = f;
                ch[t][c] = g;
                slot = slot + 1 == m ? 0 : slot + 1;
            }
        }
        __syncthreads();
        ms_flush(a.pg, ch, ln, k);
        __syncthreads();
    }
    if (ok) a.z[r * a.n_motifs + a.q0 + q] = f;                    // F[L]; 1.0 for a record shorter than the motif
}

__global__ __launch_bounds__(MS_LANES) void k_ms_backward(const MsArgs a)
{
    __shared__ double ca[MS_LANES][MS_ROW];
    __shared__ double cg[MS_LANES][MS_ROW];
    __shared__ MsLanes ln;
    extern __shared__ double ring[];                               // [m][64]: B[j + 1] .. B[j + m] of every lane
    const int t = threadIdx.x, m = a.m;
    int64_t r = 0, n_win;
    int q = 0;
    const bool ok = ms_lane(a, r, q);
    const int64_t n_chunk = ms_lanes_setup(a, ln, ok, r, q, n_win);
    for (int s = 0; s < m; ++s) ring[s * MS_LANES + t] = 1.0;      // B[n_win] .. B[L]: 1.0 + (+0.0) each
    const double v = ok ? 1.0 / a.z[r * a.n_motifs + a.q0 + q] : 0.0;   // one rounded division per record and motif
    double b = 1.0, ns = 0.0;                                      // B[j + 1]; the sites so far
    int slot = 0;                                                  // the walk's step mod m: the slot read holds B[j + m]
    double va[MS_CHUNK], vg[MS_CHUNK];
    if (n_chunk > 0) {
        ms_fetch(a.pa, ln, n_chunk - 1, va);
        ms_fetch(a.pg, ln, n_chunk - 1, vg);
    }
    for (int64_t k = n_chunk - 1; k >= 0; --k) {
        ms_park(ca, va);
        ms_park(cg, vg);
        __syncthreads();
        if (k > 0) {                                               // in flight while this chunk is walked; chunk k - 1 of G is the forward walk's
            ms_fetch(a.pa, ln, k - 1, va);
            ms_fetch(a.pg, ln, k - 1, vg);
        }
        const int64_t left = n_win - k * MS_CHUNK;
        const int n = (int)min((int64_t)MS_CHUNK, left);
#pragma unroll
        for (int c = MS_CHUNK - 1; c >= 0; --c) {
            if (c < n) {
                const double bm = ring[slot * MS_LANES + t];       // B[j + m]
                const double h = ca[t][c] * bm;
                const double st = (cg[t][c] * bm) * v;             // ((F[j] a[j]) B[j + m]) v
                b = b + h;                                         // B[j]
                ns = ns + st;
                ring[slot * MS_LANES + t] = b;
                cg[t][c] = st;
                slot = slot + 1 == m ? 0 : slot + 1;
            }
        }
        __syncthreads();
        ms_flush(a.pg, cg, ln, k);
        __syncthreads();
    }
    if (ok && a.nsites) a.nsites[r * a.n_motifs + a.q0 + q] = ns;
}

// ---- (d) cover and events ---------------------------------------------------------------------------------------------
// the events of a tile under one motif wait here and leave with one returning atomic (k_fp_tiles' queue)
struct MsQueue {
    unsigned long long base;
    double cover[MS_SLOTS];
    uint16_t at[MS_SLOTS];
    int n;
};
struct MsNoQueue {};

template <bool EVENTS>
__global__ __launch_bounds__(BLOCK) void k_ms_cover(const MsArgs a)
{
    __shared__ double wl[MS_SLOTS];
    __shared__ std::conditional_t<EVENTS, MsQueue, MsNoQueue> qu;
    const int t = threadIdx.x, m = a.m;
    const int64_t r = occ_record(a.tile_start, a.r0, a.r1, a.tile_base + (int64_t)blockIdx.x);
    const int64_t L = a.rec_len[r], off = a.rec_off[r];
    const int64_t t0 = (a.tile_base + (int64_t)blockIdx.x - a.tile_start[r]) * a.tile;
    const int n_tp = (int)min((int64_t)a.tile, L - t0);
    const int64_t w0 = t0 - (m - 1);                               // the window of slot 0: may be < 0
    const int64_t n_win = L - m + 1;
    const int n_slot = n_tp + m - 1;                               // <= MS_SLOTS
    const int64_t p0 = off + t0;                                   // the tile's first position, in the stream
    for (int q = 0; q < a.nq; ++q) {
        if (q != 0) __syncthreads();                               // the adders (and the queue) of the last motif are done
        const double *g = a.pg + (int64_t)q * a.span + (off - a.base);
#pragma unroll
        for (int j = 0; j < MS_WPL; ++j) {
            const int i = t + j * BLOCK;
            const int64_t s = w0 + i;
            if (i < n_slot) wl[i] = (s >= 0 && s < n_win) ? g[s] : 0.0;
        }
        if constexpr (EVENTS)
            if (t == 0) qu.n = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MS_WPL; ++j) {
            const int i = t + j * BLOCK;                           // position i of the tile: its windows are slots i .. i + m - 1
            if (i < n_tp) {
                const double st = wl[i + m - 1];
                double c = 0.0;
                if (EVENTS || a.cover)
                    for (int d = 0; d < m; ++d) c = c + wl[i + d];
                if constexpr (EVENTS) {
                    if (c > a.thr) {                               // strict: NaN never passes
                        const int z = atomicAdd(&qu.n, 1);         // LDS; at most n_tp <= MS_SLOTS per motif
                        qu.at[z] = (uint16_t)i;
                        qu.cover[z] = c;
                    }
                } else {
                    const int64_t p = (int64_t)(a.q0 + q) * a.n_pos + p0 + i;
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
                        a.ev_key[slot] = (int64_t)(a.q0 + q) * a.n_pos + p0 + at;
                        a.ev_cover[slot] = qu.cover[i];
                        a.ev_start[slot] = wl[at + m - 1];
                    }
                }
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static int64_t ms_scratch_cap()
{
    if (const char *e = std::getenv("PFMSCAN_MULTISITE_SCRATCH_DOUBLES")) return std::max<int64_t>(2, std::atoll(e));
    return MS_SCRATCH_DOUBLES;
}

// Launches on st, does not wait.  At least one table is given; d_codes where seq_tables is, d_codes2 where struct_tables is.
// d_lam: device.  d_z, d_nsites, d_windows may be null.  pf: the stream is an averaged-structure profile; struct_tables is then
// pf->struct_tables ([n_motifs][m][7]), seq_tables / d_codes the letter part of joint mode or null.  Only the terms launch differs.
static int ms_run(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                  const uint8_t *d_codes, const uint8_t *d_codes2, const OccRecords &rec, const double *d_lam, const FpOut &o, double *d_z,
                  double *d_nsites, int64_t *d_windows, hipStream_t st, const OccProfile *pf = nullptr)
{
    int rc;
    const bool pair = !pf && seq_tables && struct_tables;
    const int64_t pairs = rec.n_rec * n_motifs;
    const double *tables = seq_tables ? seq_tables : struct_tables;   // one table: its stream is the first strip
    const uint8_t *codes = seq_tables ? d_codes : d_codes2;
    if (!d_z) {                                                    // the backward walk divides by it
        if ((rc = ensure(ctx, ctx->exp_occ, (size_t)pairs * 8))) return rc;
        d_z = (double *)ctx->exp_occ.p;
    }
    if (d_windows) HIP_TRY(ctx, hipMemsetAsync(d_windows, 0, (size_t)rec.n_rec * 8, st));
    const int tile = MS_SLOTS - (m - 1);
    std::vector<int64_t> tiles;
    if (fp_tile_prefix(rec.len, rec.n_rec, tile, tiles) < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many positions for one call");
    int64_t need = 0;
    const std::vector<MsPass> plan = ms_plan(rec.off, rec.len, rec.n_rec, n_motifs, ms_scratch_cap(), need);
    for (const MsPass &p : plan)
        if (((p.r1 - p.r0) * p.nq + MS_LANES - 1) / MS_LANES > 0x7FFFFFFF) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many records for one pass");
    if ((rc = ensure(ctx, ctx->exp_out, std::max<size_t>((size_t)need * 8, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->fp_idx, tiles.size() * 8))) return rc;
    if ((rc = upload(ctx, ctx->fp_idx.p, tiles.data(), tiles.size() * 8, st))) return rc;
    MsArgs a{};
    if (pf) {
        if ((rc = occ_upload_tables(ctx, seq_tables, pf->struct_tables, (size_t)n_motifs * m * 7 * sizeof(double), n_motifs, m, st, a.tables, a.tables2)))
            return rc;
        a.profile = (const unsigned char *)pf->d_profile;
        a.dtype = pf->dtype;
        a.joint = seq_tables != nullptr;
    } else if ((rc = occ_upload_tables(ctx, tables, pair ? struct_tables : nullptr, (size_t)n_motifs * m * 8 * sizeof(double), n_motifs, m, st, a.tables,
                                       a.tables2))) {
        return rc;
    }
    a.codes = pf ? d_codes : codes;
    a.codes2 = pair ? d_codes2 : nullptr;
    a.rec_off = rec.d_off;
    a.rec_len = rec.d_len;
    a.tile_start = (const int64_t *)ctx->fp_idx.p;
    a.lam = d_lam;
    a.n_pos = rec.n_pos;
    a.n_motifs = n_motifs;
    a.m = m;
    a.nl = seq_tables ? 4 : PFMSCAN_NSTRUCT;
    a.tile = tile;
    a.z = d_z;
    a.nsites = d_nsites;
    a.start = o.start;
    a.cover = o.cover;
    a.thr = o.thr;
    a.capacity = o.capacity;
    a.ev_key = o.ev_key;
    a.ev_cover = o.ev_cover;
    a.ev_start = o.ev_start;
    a.ev_count = o.ev_count;
    const size_t ring = (size_t)m * MS_LANES * sizeof(double);
    for (const MsPass &p : plan) {
        a.r0 = p.r0;
        a.r1 = p.r1;
        a.q0 = p.q0;
        a.nq = p.nq;
        a.base = p.base;
        a.span = p.span;
        a.tile_base = tiles[p.r0];
        a.pa = (double *)ctx->exp_out.p;
        a.pg = a.pa + (int64_t)p.nq * p.span;
        a.windows = p.q0 == 0 ? reinterpret_cast<unsigned long long *>(d_windows) : nullptr;
        const int64_t n_tiles = tiles[p.r1] - tiles[p.r0];
        const dim3 tgrid((unsigned)n_tiles), lgrid((unsigned)(((p.r1 - p.r0) * p.nq + MS_LANES - 1) / MS_LANES));
        if (n_tiles != 0) ms_launch_terms(a, tgrid, st);
        hipLaunchKernelGGL(k_ms_forward, lgrid, dim3(MS_LANES), ring, st, a);   // also for records without a position: Z = 1.0
        hipLaunchKernelGGL(k_ms_backward, lgrid, dim3(MS_LANES), ring, st, a);
        if (n_tiles != 0) {
            if (o.events) hipLaunchKernelGGL((k_ms_cover<true>), tgrid, dim3(BLOCK), 0, st, a);
            else hipLaunchKernelGGL((k_ms_cover<false>), tgrid, dim3(BLOCK), 0, st, a);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(ctx, e, "k_ms_*");
    }
    return PFMSCAN_OK;
}

// the checks of all four entry points up to "n_rec == 0 or n_motifs == 0: nothing to do", in the order of pfmscan_footprint_*
static int ms_check(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m, int64_t n_pos,
                    int64_t n_rec, const double *lam)
{
    if (int rc = occ_check_base(ctx, who, m, nullptr, n_motifs, n_rec, n_pos, seq_tables || struct_tables ? nullptr : ": seq_tables and struct_tables are both NULL"))
        return rc;
    if (!lam) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": lam is NULL");
    return PFMSCAN_OK;
}

// both _dev forms
static int ms_dev(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                  const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec,
                  const double *d_lam, const FpOut &o, double *d_z, double *d_nsites, int64_t *d_windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = ms_check(ctx, who, seq_tables, struct_tables, n_motifs, m, n_pos, n_rec, d_lam)) return rc;
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
    return ms_run(ctx, who, seq_tables, struct_tables, n_motifs, m, d_codes, d_codes2, rec, d_lam, o, d_z, d_nsites, d_windows, ctx->stream);
}

// the checks of both _staged forms of what is staged
static int ms_staged_check(pfmscan_ctx *ctx, const char *who, const double *seq_tables, const double *struct_tables)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (ctx->staged_n > 0 && seq_tables && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes are staged");
    if (ctx->staged_n > 0 && struct_tables && !ctx->staged_codes2)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes2 are staged (pfmscan_stage_codes2)");
    return PFMSCAN_OK;
}

// a _staged form's lam: up into ctx->exp_inv on ctx->stream
static int ms_lam_up(pfmscan_ctx *ctx, const double *lam, int64_t n_rec, const double *&d_lam)
{
    int rc;
    if ((rc = ensure(ctx, ctx->exp_inv, (size_t)n_rec * 8))) return rc;
    if ((rc = upload(ctx, ctx->exp_inv.p, lam, (size_t)n_rec * 8, ctx->stream))) return rc;
    d_lam = (const double *)ctx->exp_inv.p;
    return PFMSCAN_OK;
}

// ---- on averaged-structure profiles: the checks are pfmscan_footprint_profile_*'s (without mode), then lam ----------------------
static int msp_check(pfmscan_ctx *ctx, const char *who, const double *struct_tables, int n_motifs, int m, int profile_dtype, int64_t n_pos,
                     int64_t n_rec, const double *lam)
{
    const char *own = profile_dtype != PFMSCAN_PROFILE_F32 && profile_dtype != PFMSCAN_PROFILE_F64 ? ": profile_dtype must be PFMSCAN_PROFILE_F32 or F64" : nullptr;
    if (int rc = occ_check_base(ctx, who, m, own, n_motifs, n_rec, n_pos, nullptr)) return rc;
    if (!struct_tables)
        return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": struct_tables is NULL (the multi-site model of a profile's letters is pfmscan_multisite_* on the codes)");
    if (!lam) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": lam is NULL");
    return PFMSCAN_OK;
}

// both _dev forms
static int msp_dev(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                   const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len,
                   int64_t n_rec, const double *d_lam, const FpOut &o, double *d_z, double *d_nsites, int64_t *d_windows)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (int rc = msp_check(ctx, who, struct_tables, n_motifs, m, profile_dtype, n_pos, n_rec, d_lam)) return rc;
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
    const OccProfile pf{struct_tables, d_profile, profile_dtype};
    return ms_run(ctx, who, seq_tables, struct_tables, n_motifs, m, d_codes, nullptr, rec, d_lam, o, d_z, d_nsites, d_windows, ctx->stream, &pf);
}

// the checks of both _staged forms, up to "n_rec == 0 or n_motifs == 0: nothing to do" without the outputs' own
static int msp_staged_check(pfmscan_ctx *ctx, const char *who, const double *struct_tables, const double *seq_tables, int n_motifs, int m, int64_t n_rec,
                            const double *lam)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (!ctx->staged_profile) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no profile is staged");
    if (seq_tables && !ctx->staged_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": seq_tables (joint mode) needs staged codes");
    return msp_check(ctx, who, struct_tables, n_motifs, m, ctx->staged_dtype, ctx->staged_n, n_rec, lam);
}

}  // namespace pfmscan

using namespace pfmscan;

extern "C" {

int pfmscan_multisite_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, const uint8_t *d_codes,
                          const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off, const int64_t *d_rec_len, int64_t n_rec,
                          const double *d_lam, double *d_start, double *d_cover, double *d_z, double *d_nsites, int64_t *d_windows)
{
    const FpOut o{d_start, d_cover, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    return ms_dev(ctx, "pfmscan_multisite_dev", seq_tables, struct_tables, n_motifs, m, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec, d_lam, o,
                  d_z, d_nsites, d_windows);
}

int pfmscan_multisite_events_dev(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                 const uint8_t *d_codes, const uint8_t *d_codes2, int64_t n_pos, const int64_t *d_rec_off,
                                 const int64_t *d_rec_len, int64_t n_rec, const double *d_lam, double thr, int64_t capacity, int64_t *d_ev_key,
                                 double *d_ev_cover, double *d_ev_start, uint64_t *d_ev_count, double *d_z, double *d_nsites, int64_t *d_windows)
{
    const FpOut o{nullptr, nullptr, true, thr, capacity, d_ev_key, d_ev_cover, d_ev_start, reinterpret_cast<unsigned long long *>(d_ev_count)};
    return ms_dev(ctx, "pfmscan_multisite_events_dev", seq_tables, struct_tables, n_motifs, m, d_codes, d_codes2, n_pos, d_rec_off, d_rec_len, n_rec,
                  d_lam, o, d_z, d_nsites, d_windows);
}

int pfmscan_multisite_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m, const int64_t *rec_off,
                             const int64_t *rec_len, int64_t n_rec, const double *lam, double *start, double *cover, double *z, double *nsites,
                             int64_t *windows)
{
    const char *who = "pfmscan_multisite_staged";
    if (int rc = ms_staged_check(ctx, who, seq_tables, struct_tables)) return rc;
    const int64_t n_pos = ctx->staged_n;
    if (int rc = ms_check(ctx, who, seq_tables, struct_tables, n_motifs, m, n_pos, n_rec, lam)) return rc;
    if (!start && !cover) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": start and cover are both NULL");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const double *d_lam;
    if ((rc = ms_lam_up(ctx, lam, n_rec, d_lam))) return rc;
    const size_t plane = (size_t)n_motifs * (size_t)n_pos, pairs = (size_t)n_rec * n_motifs;
    if ((rc = ensure(ctx, ctx->fp_out, std::max<size_t>((2 * plane + 2 * pairs + (size_t)n_rec) * 8, 16)))) return rc;
    double *d_base = (double *)ctx->fp_out.p;
    double *d_start = start ? d_base : nullptr;
    double *d_cover = cover ? d_base + plane : nullptr;
    double *d_z = z ? d_base + 2 * plane : nullptr;
    double *d_ns = nsites ? d_base + 2 * plane + pairs : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_base + 2 * plane + 2 * pairs) : nullptr;
    // positions in no record of the table are +0.0
    if (d_start && plane) HIP_TRY(ctx, hipMemsetAsync(d_start, 0, plane * 8, ctx->stream));
    if (d_cover && plane) HIP_TRY(ctx, hipMemsetAsync(d_cover, 0, plane * 8, ctx->stream));
    const FpOut o{d_start, d_cover, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    if ((rc = ms_run(ctx, who, seq_tables, struct_tables, n_motifs, m, (const uint8_t *)ctx->codes.p, (const uint8_t *)ctx->codes2.p, rec, d_lam, o, d_z,
                     d_ns, d_win, ctx->stream)))
        return rc;
    return occ_copy_home(ctx, {{start, d_start, plane * 8}, {cover, d_cover, plane * 8}, {z, d_z, pairs * 8}, {nsites, d_ns, pairs * 8},
                               {windows, d_win, (size_t)n_rec * 8}});
}

int pfmscan_multisite_events_staged(pfmscan_ctx *ctx, const double *seq_tables, const double *struct_tables, int n_motifs, int m,
                                    const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const double *lam, double thr, int64_t capacity,
                                    int64_t *ev_key, double *ev_cover, double *ev_start, int64_t *n_events, double *z, double *nsites,
                                    int64_t *windows)
{
    const char *who = "pfmscan_multisite_events_staged";
    if (int rc = ms_staged_check(ctx, who, seq_tables, struct_tables)) return rc;
    const int64_t n_pos = ctx->staged_n;
    if (int rc = ms_check(ctx, who, seq_tables, struct_tables, n_motifs, m, n_pos, n_rec, lam)) return rc;
    if (int rc = fp_check_events(ctx, who, thr, capacity, n_events, ev_key, ev_cover, ev_start)) return rc;
    *n_events = 0;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const double *d_lam;
    if ((rc = ms_lam_up(ctx, lam, n_rec, d_lam))) return rc;
    const size_t pairs = (size_t)n_rec * n_motifs;
    FpOut o;
    double *d_both;                                                // z, then nsites
    int64_t *d_win;
    if ((rc = fp_events_room(ctx, thr, capacity, 2 * pairs, (size_t)n_rec, true, windows != nullptr, o, d_both, d_win))) return rc;
    double *d_z = z ? d_both : nullptr, *d_ns = nsites ? d_both + pairs : nullptr;
    if ((rc = ms_run(ctx, who, seq_tables, struct_tables, n_motifs, m, (const uint8_t *)ctx->codes.p, (const uint8_t *)ctx->codes2.p, rec, d_lam, o, d_z,
                     d_ns, d_win, ctx->stream)))
        return rc;
    if (nsites) HIP_TRY(ctx, hipMemcpyAsync(nsites, d_ns, pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
    return fp_events_home(ctx, who, o, ev_key, ev_cover, ev_start, n_events, {z, d_z, pairs * 8}, {windows, d_win, (size_t)n_rec * 8});
}

int pfmscan_multisite_profile_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                  const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off,
                                  const int64_t *d_rec_len, int64_t n_rec, const double *d_lam, double *d_start, double *d_cover, double *d_z,
                                  double *d_nsites, int64_t *d_windows)
{
    const FpOut o{d_start, d_cover, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    return msp_dev(ctx, "pfmscan_multisite_profile_dev", struct_tables, seq_tables, n_motifs, m, d_codes, d_profile, profile_dtype, n_pos, d_rec_off,
                   d_rec_len, n_rec, d_lam, o, d_z, d_nsites, d_windows);
}

int pfmscan_multisite_profile_events_dev(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                         const uint8_t *d_codes, const void *d_profile, int profile_dtype, int64_t n_pos, const int64_t *d_rec_off,
                                         const int64_t *d_rec_len, int64_t n_rec, const double *d_lam, double thr, int64_t capacity,
                                         int64_t *d_ev_key, double *d_ev_cover, double *d_ev_start, uint64_t *d_ev_count, double *d_z,
                                         double *d_nsites, int64_t *d_windows)
{
    const FpOut o{nullptr, nullptr, true, thr, capacity, d_ev_key, d_ev_cover, d_ev_start, reinterpret_cast<unsigned long long *>(d_ev_count)};
    return msp_dev(ctx, "pfmscan_multisite_profile_events_dev", struct_tables, seq_tables, n_motifs, m, d_codes, d_profile, profile_dtype, n_pos,
                   d_rec_off, d_rec_len, n_rec, d_lam, o, d_z, d_nsites, d_windows);
}

int pfmscan_multisite_profile_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                     const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const double *lam, double *start, double *cover,
                                     double *z, double *nsites, int64_t *windows)
{
    const char *who = "pfmscan_multisite_profile_staged";
    if (int rc = msp_staged_check(ctx, who, struct_tables, seq_tables, n_motifs, m, n_rec, lam)) return rc;
    if (!start && !cover) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": start and cover are both NULL");
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const double *d_lam;
    if ((rc = ms_lam_up(ctx, lam, n_rec, d_lam))) return rc;
    const int64_t n_pos = ctx->staged_n;
    const size_t plane = (size_t)n_motifs * (size_t)n_pos, pairs = (size_t)n_rec * n_motifs;
    if ((rc = ensure(ctx, ctx->fp_out, std::max<size_t>((2 * plane + 2 * pairs + (size_t)n_rec) * 8, 16)))) return rc;
    double *d_base = (double *)ctx->fp_out.p;
    double *d_start = start ? d_base : nullptr;
    double *d_cover = cover ? d_base + plane : nullptr;
    double *d_z = z ? d_base + 2 * plane : nullptr;
    double *d_ns = nsites ? d_base + 2 * plane + pairs : nullptr;
    int64_t *d_win = windows ? (int64_t *)(d_base + 2 * plane + 2 * pairs) : nullptr;
    // positions in no record of the table are +0.0
    if (d_start && plane) HIP_TRY(ctx, hipMemsetAsync(d_start, 0, plane * 8, ctx->stream));
    if (d_cover && plane) HIP_TRY(ctx, hipMemsetAsync(d_cover, 0, plane * 8, ctx->stream));
    const FpOut o{d_start, d_cover, false, 0.0, 0, nullptr, nullptr, nullptr, nullptr};
    const OccProfile pf{struct_tables, ctx->profile.p, ctx->staged_dtype};
    if ((rc = ms_run(ctx, who, seq_tables, struct_tables, n_motifs, m, (const uint8_t *)ctx->codes.p, nullptr, rec, d_lam, o, d_z, d_ns, d_win, ctx->stream,
                     &pf)))
        return rc;
    return occ_copy_home(ctx, {{start, d_start, plane * 8}, {cover, d_cover, plane * 8}, {z, d_z, pairs * 8}, {nsites, d_ns, pairs * 8},
                               {windows, d_win, (size_t)n_rec * 8}});
}

int pfmscan_multisite_profile_events_staged(pfmscan_ctx *ctx, const double *struct_tables, const double *seq_tables, int n_motifs, int m,
                                            const int64_t *rec_off, const int64_t *rec_len, int64_t n_rec, const double *lam, double thr,
                                            int64_t capacity, int64_t *ev_key, double *ev_cover, double *ev_start, int64_t *n_events, double *z,
                                            double *nsites, int64_t *windows)
{
    const char *who = "pfmscan_multisite_profile_events_staged";
    if (int rc = msp_staged_check(ctx, who, struct_tables, seq_tables, n_motifs, m, n_rec, lam)) return rc;
    if (int rc = fp_check_events(ctx, who, thr, capacity, n_events, ev_key, ev_cover, ev_start)) return rc;
    *n_events = 0;
    if (n_rec == 0 || n_motifs == 0) return PFMSCAN_OK;
    if (!rec_off || !rec_len) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL record table");
    int rc;
    OccRecords rec;
    if ((rc = occ_records_up(ctx, who, rec_off, rec_len, n_rec, rec))) return rc;
    const double *d_lam;
    if ((rc = ms_lam_up(ctx, lam, n_rec, d_lam))) return rc;
    const size_t pairs = (size_t)n_rec * n_motifs;
    FpOut o;
    double *d_both;                                                // z, then nsites
    int64_t *d_win;
    if ((rc = fp_events_room(ctx, thr, capacity, 2 * pairs, (size_t)n_rec, true, windows != nullptr, o, d_both, d_win))) return rc;
    double *d_z = z ? d_both : nullptr, *d_ns = nsites ? d_both + pairs : nullptr;
    const OccProfile pf{struct_tables, ctx->profile.p, ctx->staged_dtype};
    if ((rc = ms_run(ctx, who, seq_tables, struct_tables, n_motifs, m, (const uint8_t *)ctx->codes.p, nullptr, rec, d_lam, o, d_z, d_ns, d_win, ctx->stream,
                     &pf)))
        return rc;
    if (nsites) HIP_TRY(ctx, hipMemcpyAsync(nsites, d_ns, pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
    return fp_events_home(ctx, who, o, ev_key, ev_cover, ev_start, n_events, {z, d_z, pairs * 8}, {windows, d_win, (size_t)n_rec * 8});
}

}  // extern "C"
