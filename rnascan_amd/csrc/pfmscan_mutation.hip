// pfmscan_mutation.hip -- in-silico mutagenesis: which single-letter changes create or destroy a site.
//
// score(s | p->a) is what the letters scan would write at window s if codes[p] were a: 0.0 (double), += T[k][code(s + k)] for k
// ascending with every addition rounded, then (float) (_pwm.c:34-68); NaN when the window holds a code >= 4 or runs past the
// stream.  best[p][a] is the greatest non-NaN score over the windows that cover p, compared as float32; ties go to the lowest
// start; where[p][a] = p - s of that window (-1: no window).  Positions whose code is not a letter (>= 4) are never
// substituted: all four columns NaN / -1.
//
// The sum is sequential, so for offset j = p - s the first j additions of a window do not depend on the letter at p: the
// partial sum over k < j is taken ONCE and shared by the four columns, only the tail k >= j is added per letter.  Every
// addition that the plain scan of the mutated stream makes is made here, on the same operands in the same order: same bits.
//
//   k_mutmap<M, EVENTS>        width as a compile-time constant (1 .. MUT_FIXED_MAX): the 2M - 1 codes around a position sit in
//                              registers that are indexed by constants only (static_for), every table row offset is an
//                              immediate of its ds_read_b64, T[j][a] of the substituted letter is a scalar operand
//   k_mutmap_rolled<EVENTS>    any width up to PFMSCAN_MAX_M: the neighbourhood stays in LDS and is indexed there
// Both stage a tile of codes with a halo of MUT_HALO bytes on BOTH sides (the windows over p start up to m - 1 before it and
// end up to m - 1 after it); positions before the stream and behind it read as separators.
//   dense   best float [n_pos][4] as one 16-byte store per position, where int8 [n_pos][4] as one 4-byte store
//   EVENTS  nothing dense: every (p, a != codes[p]) whose alt best passes thr while the ref best does not (gain), or the
//           reverse (loss), waits in an LDS queue and is appended through the HitShard protocol, one returning atomic per tile
//   k_variants                 a list of variants x a library of letter tables of one width: a wave takes a variant (its
//                              codes are wave-uniform), a lane takes a motif; the tables of a chunk of motifs sit in LDS
//                              transposed ([row][letter][motif]: consecutive lanes, consecutive words)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "pfmscan_hits.hpp"
#include "pfmscan_device.hpp"

namespace pfmscan {

constexpr int MUT_TILE = 1024;                        // positions per workgroup
constexpr int MUT_ROUNDS = MUT_TILE / BLOCK;
constexpr int MUT_HALO = 64;                          // >= PFMSCAN_MAX_M - 1, multiple of 16: the tile's halo on either side
constexpr int MUT_FIXED_MAX = 20;                     // widest compile-time instantiation (the reference's example PFMs are 18 wide)
static_assert(MUT_HALO >= PFMSCAN_MAX_M - 1 && MUT_HALO % 16 == 0 && MUT_TILE % 16 == 0, "halo");

struct MutArgs {
    const uint8_t *codes;        // [n_pos]
    int64_t n_pos;
    const double *table;         // [m][8] device
    int m;
    float *best;                 // dense: [n_pos][4]
    int8_t *where;               // dense: [n_pos][4] or null
    double thr;                  // events
    int64_t capacity;
    int64_t *ev_key;             // [capacity] 4 p + a
    float *ev_ref, *ev_alt;      // [capacity]
    unsigned long long *ev_count;
};

// codes [tile0 - MUT_HALO, tile0 + MUT_TILE + MUT_HALO) -> cbuf as 16-byte vectors; outside [0, n_pos): separators.
// tile0 is a multiple of MUT_TILE and the base is 16-byte aligned, so a vector lies before the stream entirely or not at all.
__device__ __forceinline__ void mut_stage(uint8_t *cbuf, const uint8_t *__restrict__ codes, int64_t tile0, int64_t n_pos)
{
    constexpr int NVEC = (MUT_TILE + 2 * MUT_HALO) / 16;
    static_assert(NVEC <= BLOCK, "one vector per thread");
    if (threadIdx.x < NVEC) {
        const int64_t p = tile0 - MUT_HALO + 16 * (int64_t)threadIdx.x;
        u32x4 v = {0x07070707u, 0x07070707u, 0x07070707u, 0x07070707u};
        if (p >= 0 && p + 16 <= n_pos) {
            v = *reinterpret_cast<const u32x4 *>(codes + p);
        } else if (p >= 0 && p < n_pos) {
            uint32_t t[4] = {0x07070707u, 0x07070707u, 0x07070707u, 0x07070707u};
            for (int b = 0; b < 16; ++b)
                if (p + b < n_pos) t[b >> 2] = (t[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)codes[p + b] << (8 * (b & 3)));
            v = u32x4{t[0], t[1], t[2], t[3]};
        }
        v &= 0x07070707u;
        *reinterpret_cast<u32x4 *>(cbuf + 16 * threadIdx.x) = v;
    }
}

// the letter table -> LDS; columns 4 .. 7 read as NaN whatever the motif holds there (codes >= 4 are foreign to this scan)
__device__ __forceinline__ void mut_table(double *tbl, const double *__restrict__ table, int m)
{
    for (int i = threadIdx.x; i < m * 8; i += BLOCK) tbl[i] = (i & 4) ? __builtin_nan("") : table[i];
}

// greatest non-NaN float32 so far; called from the lowest start on, so a tie keeps the lowest start
__device__ __forceinline__ void mut_take(float f, int j, float &best, int &wh)
{
    if (f == f && !(f <= best)) {
        best = f;
        wh = j;
    }
}

// The events of a workgroup's tile wait in LDS and leave with ONE returning atomic per workgroup: the _dev contract has a
// single counter word, and one atomic per wave and round saturated it (41 ms at C2 size where a percent of the positions has
// an event; a word takes ~88 atomics per microsecond).  A tile has at most 3 events per position.
constexpr int EVQ_CAP = MUT_TILE * 3;
struct MutEventQueue {
    unsigned long long base;     // the workgroup's first slot, thread 0 -> everybody
    uint32_t key[EVQ_CAP];       // 4 * (position - tile0) + letter
    float ref[EVQ_CAP], alt[EVQ_CAP];
    int n;
};

// gain / loss events of one position (mask: bit a set = column a is an event) -> the queue; every lane of the wave calls
__device__ __forceinline__ void mut_emit(MutEventQueue &q, uint32_t mask, int local, float ref, float b0, float b1, float b2, float b3)
{
    if (__builtin_amdgcn_ballot_w64(mask != 0) == 0) return;           // wave-uniform
    const int lane = threadIdx.x & 63;
    const int cnt = __popc(mask);
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    const int total = __shfl(incl, 63);
    int first = 0;
    if (lane == 0) first = atomicAdd(&q.n, total);                     // LDS
    int slot = __builtin_amdgcn_readfirstlane(first) + incl - cnt;
    const float alt[4] = {b0, b1, b2, b3};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (mask & (1u << c)) {
            q.key[slot] = (uint32_t)(4 * local + c);
            q.ref[slot] = ref;
            q.alt[slot] = alt[c];
            ++slot;
        }
    }
}

// the tile's events -> the caller's arrays (HitShard protocol: slots at or beyond the capacity are counted, never stored); all 256 threads
__device__ __forceinline__ void mut_flush(const MutArgs &a, MutEventQueue &q, int64_t tile0)
{
    __syncthreads();
    const int n = q.n;
    if (n == 0) return;                                                // uniform: read behind the barrier
    const HitShard shard{a.ev_count, 1, a.capacity};
    if (threadIdx.x == 0) q.base = shard.reserve((unsigned long long)n);
    __syncthreads();
    const unsigned long long base = q.base;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const unsigned long long slot = base + (unsigned long long)i;
        if (shard.in_range(slot)) {
            a.ev_key[slot] = 4 * tile0 + (int64_t)q.key[i];
            a.ev_ref[slot] = q.ref[i];
            a.ev_alt[slot] = q.alt[i];
        }
    }
}

// what a position reports: the dense row, or its events
template <bool EVENTS>
__device__ __forceinline__ void mut_report(const MutArgs &a, MutEventQueue *q, int local, int64_t p, int c, float b0, float b1, float b2, float b3, int w0, int w1, int w2, int w3)
{
    const bool inside = p < a.n_pos;
    if (c >= 4 || !inside) {
        b0 = b1 = b2 = b3 = __builtin_nanf("");
        w0 = w1 = w2 = w3 = -1;
    }
    if constexpr (EVENTS) {
        const float ref = c == 0 ? b0 : c == 1 ? b1 : c == 2 ? b2 : b3;
        const bool pr = (double)ref > a.thr;                            // strict: NaN and -inf never pass
        uint32_t mask = 0;
        if (inside && c < 4) {
            mask = (((double)b0 > a.thr) != pr ? 1u : 0u) | (((double)b1 > a.thr) != pr ? 2u : 0u) |
                   (((double)b2 > a.thr) != pr ? 4u : 0u) | (((double)b3 > a.thr) != pr ? 8u : 0u);
            mask &= ~(1u << c);
        }
        mut_emit(*q, mask, local, ref, b0, b1, b2, b3);
    } else {
        if (inside) {
            const f32x4 r = {b0, b1, b2, b3};
            reinterpret_cast<f32x4 *>(a.best)[p] = r;
            if (a.where)
                reinterpret_cast<uint32_t *>(a.where)[p] = (uint32_t)(w0 & 0xFF) | (uint32_t)(w1 & 0xFF) << 8 | (uint32_t)(w2 & 0xFF) << 16 | (uint32_t)(w3 & 0xFF) << 24;
        }
    }
}

template <int M, bool EVENTS>
__global__ __launch_bounds__(BLOCK) void k_mutmap(const MutArgs a)
{
    static_assert(M >= 1 && M <= MUT_FIXED_MAX, "width outside this kernel's range");
    constexpr int NB = 2 * M - 1;                     // codes around a position: offsets -(M - 1) .. M - 1
    __shared__ __align__(16) double tbl[M * 8];
    __shared__ __align__(16) uint8_t cbuf[MUT_TILE + 2 * MUT_HALO];
    __shared__ MutEventQueue evq;                       // EVENTS only: the dense kernels never name it and get no LDS for it
    const int64_t tile0 = (int64_t)blockIdx.x * MUT_TILE;
    if constexpr (EVENTS) {
        if (threadIdx.x == 0) evq.n = 0;
    }
    mut_stage(cbuf, a.codes, tile0, a.n_pos);
    mut_table(tbl, a.table, M);
    __syncthreads();

    typedef const volatile __attribute__((address_space(3))) double *lds_f64;   // one ds_read_b64 per look-up (pfmscan_letters_fixed.hip)
    typedef const __attribute__((address_space(3))) char *lds_bytes;
    const lds_bytes tb = (lds_bytes)reinterpret_cast<const char *>(tbl);
    // T[j][a] of the substituted letter: uniform addresses in the constant address space, i.e. scalar loads and scalar operands
    const __attribute__((address_space(4))) double *T = (const __attribute__((address_space(4))) double *)a.table;
#pragma unroll 1
    for (int it = 0; it < MUT_ROUNDS; ++it) {
        const int local = it * BLOCK + (int)threadIdx.x;
        const uint8_t *nbp = cbuf + MUT_HALO + local - (M - 1);
        uint32_t adr[NB];                             // byte offset of the code's column in a table row
        static_for<0, NB>([&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value;
            adr[q] = (uint32_t)nbp[q] << 3;
        });
        const int c = (int)(adr[M - 1] >> 3);
        const float nanf_ = __builtin_nanf("");
        float b0 = nanf_, b1 = nanf_, b2 = nanf_, b3 = nanf_;
        int w0 = -1, w1 = -1, w2 = -1, w3 = -1;
        static_for<0, M>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = M - 1 - decltype(jc)::value;              // the lowest start first; window letter k is adr[M - 1 - j + k]
            double pre = 0.0;
            static_for<0, j>([&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                pre += *(lds_f64)(tb + k * 64 + adr[M - 1 - j + k]);
            });
            double s0 = pre + T[j * 8 + 0], s1 = pre + T[j * 8 + 1], s2 = pre + T[j * 8 + 2], s3 = pre + T[j * 8 + 3];
            static_for<j + 1, M>([&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                const double t = *(lds_f64)(tb + k * 64 + adr[M - 1 - j + k]);
                s0 += t;
                s1 += t;
                s2 += t;
                s3 += t;
            });
            mut_take((float)s0, j, b0, w0);
            mut_take((float)s1, j, b1, w1);
            mut_take((float)s2, j, b2, w2);
            mut_take((float)s3, j, b3, w3);
        });
        mut_report<EVENTS>(a, EVENTS ? &evq : nullptr, local, tile0 + local, c, b0, b1, b2, b3, w0, w1, w2, w3);
    }
    if constexpr (EVENTS) mut_flush(a, evq, tile0);
}

template <bool EVENTS>
__global__ __launch_bounds__(BLOCK) void k_mutmap_rolled(const MutArgs a)
{
    __shared__ __align__(16) double tbl[PFMSCAN_MAX_M * 8];
    __shared__ __align__(16) uint8_t cbuf[MUT_TILE + 2 * MUT_HALO];
    const int m = a.m;
    __shared__ MutEventQueue evq;                       // EVENTS only: the dense kernels never name it and get no LDS for it
    const int64_t tile0 = (int64_t)blockIdx.x * MUT_TILE;
    if constexpr (EVENTS) {
        if (threadIdx.x == 0) evq.n = 0;
    }
    mut_stage(cbuf, a.codes, tile0, a.n_pos);
    mut_table(tbl, a.table, m);
    __syncthreads();
    const __attribute__((address_space(4))) double *T = (const __attribute__((address_space(4))) double *)a.table;
#pragma unroll 1
    for (int it = 0; it < MUT_ROUNDS; ++it) {
        const int local = it * BLOCK + (int)threadIdx.x;
        const uint8_t *here = cbuf + MUT_HALO + local;
        const int c = here[0];
        const float nanf_ = __builtin_nanf("");
        float b0 = nanf_, b1 = nanf_, b2 = nanf_, b3 = nanf_;
        int w0 = -1, w1 = -1, w2 = -1, w3 = -1;
#pragma unroll 1
        for (int j = m - 1; j >= 0; --j) {
            const uint8_t *w = here - j;                                // the window's first letter: >= cbuf, j <= MUT_HALO - 1
            double pre = 0.0;
#pragma unroll 1
            for (int k = 0; k < j; ++k) pre += tbl[k * 8 + w[k]];
            double s0 = pre + T[j * 8 + 0], s1 = pre + T[j * 8 + 1], s2 = pre + T[j * 8 + 2], s3 = pre + T[j * 8 + 3];
#pragma unroll 1
            for (int k = j + 1; k < m; ++k) {
                const double t = tbl[k * 8 + w[k]];
                s0 += t;
                s1 += t;
                s2 += t;
                s3 += t;
            }
            mut_take((float)s0, j, b0, w0);
            mut_take((float)s1, j, b1, w1);
            mut_take((float)s2, j, b2, w2);
            mut_take((float)s3, j, b3, w3);
        }
        mut_report<EVENTS>(a, EVENTS ? &evq : nullptr, local, tile0 + local, c, b0, b1, b2, b3, w0, w1, w2, w3);
    }
    if constexpr (EVENTS) mut_flush(a, evq, tile0);
}

template <bool EVENTS> static hipError_t launch_mutmap(const MutArgs &a, hipStream_t stream)
{
    if (a.n_pos <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((a.n_pos + MUT_TILE - 1) / MUT_TILE);
    const bool rolled = std::getenv("PFMSCAN_MUTMAP_ROLLED") != nullptr;   // tests and A/B runs: the rolled kernel at every width
    switch (rolled ? 0 : a.m) {
#define MUT_WIDTH(W) case W: hipLaunchKernelGGL((k_mutmap<W, EVENTS>), dim3(grid), dim3(BLOCK), 0, stream, a); break;
    MUT_WIDTH(1) MUT_WIDTH(2) MUT_WIDTH(3) MUT_WIDTH(4) MUT_WIDTH(5) MUT_WIDTH(6) MUT_WIDTH(7) MUT_WIDTH(8) MUT_WIDTH(9) MUT_WIDTH(10)
    MUT_WIDTH(11) MUT_WIDTH(12) MUT_WIDTH(13) MUT_WIDTH(14) MUT_WIDTH(15) MUT_WIDTH(16) MUT_WIDTH(17) MUT_WIDTH(18) MUT_WIDTH(19) MUT_WIDTH(20)
#undef MUT_WIDTH
    default: hipLaunchKernelGGL((k_mutmap_rolled<EVENTS>), dim3(grid), dim3(BLOCK), 0, stream, a); break;
    }
    return hipGetLastError();
}

// ---- variants x library ------------------------------------------------------------------------------------------------
constexpr int VAR_LDS_DOUBLES = 4096;                 // table cells of one motif chunk in LDS (32 KB): chunk = 1024 / m motifs
constexpr int VAR_PER_BLOCK = 64;                     // variants per workgroup, 16 per wave

struct VarArgs {
    const uint8_t *codes;
    int64_t n_pos;
    const double *tables;        // [n_motifs][m][8] device
    int n_motifs, m, chunk;      // chunk = motifs per pass over blockIdx.y
    const int64_t *var_pos;      // [n_var]
    const uint8_t *var_alt;      // [n_var]
    int64_t n_var;
    float *ref, *alt;            // [n_var][n_motifs]
    int8_t *ref_where, *alt_where;   // [n_var][n_motifs] or null
};

__host__ __device__ constexpr int var_chunk(int m) { return VAR_LDS_DOUBLES / (4 * m); }

__global__ __launch_bounds__(BLOCK) void k_variants(const VarArgs a)
{
    __shared__ __align__(16) double lt[VAR_LDS_DOUBLES];                 // [row][letter][motif of the chunk]
    __shared__ uint16_t nb[BLOCK / 64][2 * PFMSCAN_MAX_M];               // a wave's variant: row-cell offsets of the codes at offsets -(m - 1) .. m - 1
    const int m = a.m;
    const int q0 = (int)blockIdx.y * a.chunk;
    const int nq = min(a.chunk, a.n_motifs - q0);
    for (int i = threadIdx.x; i < nq * m * 4; i += BLOCK) {
        const int q = i / (m * 4), r = i - q * (m * 4);                  // r = row * 4 + letter
        lt[r * nq + q] = a.tables[((int64_t)(q0 + q) * m + (r >> 2)) * 8 + (r & 3)];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float nanf_ = __builtin_nanf("");
    const int64_t v_end = min(a.n_var, ((int64_t)blockIdx.x + 1) * VAR_PER_BLOCK);
    for (int64_t v = (int64_t)blockIdx.x * VAR_PER_BLOCK + wave; v < v_end; v += BLOCK / 64) {   // wave-uniform
        const int64_t pos = a.var_pos[v];
        const int alt = a.var_alt[v];
        bool ok = pos >= 0 && pos < a.n_pos && alt < 4;
        int c = 7;
        if (ok) c = a.codes[pos] & 7;
        ok = ok && c < 4;
        // the codes at offsets -(m - 1) .. m - 1: to LDS as the offset of the code's cell in a table row ((code & 3) * nq doubles), the
        // foreign ones as two wave-wide bit masks (bit i = offset i - (m - 1)); a window is m consecutive entries of either
        int c0 = 0, c1 = 0;
        if (ok) {
            const int64_t p0 = pos - (m - 1) + lane, p1 = p0 + 64;
            if (lane < 2 * m - 1) c0 = (p0 >= 0 && p0 < a.n_pos) ? (a.codes[p0] & 7) : 7;
            if (lane + 64 < 2 * m - 1) c1 = (p1 >= 0 && p1 < a.n_pos) ? (a.codes[p1] & 7) : 7;
            nb[wave][lane] = (uint16_t)((c0 & 3) * nq);
            nb[wave][lane + 64] = (uint16_t)((c1 & 3) * nq);
        }
        const unsigned long long f0 = __builtin_amdgcn_ballot_w64(c0 >= 4), f1 = __builtin_amdgcn_ballot_w64(c1 >= 4);
        const unsigned long long wmask = m == 64 ? ~0ull : (1ull << m) - 1;
        const int rs = 4 * nq;                                            // doubles per table row
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int q = lane; q < nq; q += 64) {
            float br = nanf_, ba = nanf_;
            int wr = -1, wa = -1;
            if (ok) {
                const double *lq = lt + q;
#pragma unroll 1
                for (int j = m - 1; j >= 0; --j) {
                    const int start = m - 1 - j;                          // the window's first letter; <= 63
                    const unsigned long long win = start ? (f0 >> start) | (f1 << (64 - start)) : f0;
                    if (win & wmask) continue;                            // wave-uniform: a foreign letter in the window (never the variant's own: c < 4)
                    const uint16_t *w = &nb[wave][start];
                    const double *row = lq;
                    double pre = 0.0;
#pragma unroll 4
                    for (int k = 0; k < j; ++k) {
                        pre += row[w[k]];
                        row += rs;
                    }
                    double sr = pre + row[c * nq], sa = pre + row[alt * nq];
                    row += rs;
#pragma unroll 4
                    for (int k = j + 1; k < m; ++k) {
                        const double t = row[w[k]];
                        sr += t;
                        sa += t;
                        row += rs;
                    }
                    mut_take((float)sr, j, br, wr);
                    mut_take((float)sa, j, ba, wa);
                }
            }
            const int64_t o = v * a.n_motifs + q0 + q;
            a.ref[o] = br;
            a.alt[o] = ba;
            if (a.ref_where) a.ref_where[o] = (int8_t)wr;
            if (a.alt_where) a.alt_where[o] = (int8_t)wa;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                                  // nb[wave] is rewritten by the next variant
    }
}

}  // namespace pfmscan

using namespace pfmscan;

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
static int mut_check(pfmscan_ctx *ctx, const pfmscan_motif *mo, const uint8_t *d_codes, int64_t n_pos, const char *who)
{
    if (!ctx || !mo) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx or motif");
    if (mo->ctx != ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": motif belongs to another ctx");
    if (!mo->d_letters) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": the motif has no letters part");
    if (mo->m > PFMSCAN_MAX_M)
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": width " + std::to_string(mo->m) + " exceeds PFMSCAN_MAX_M (" + std::to_string(PFMSCAN_MAX_M) + ")");
    if (n_pos < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": negative n_pos");
    if (n_pos > 0 && !d_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": codes is NULL");
    if (misaligned(d_codes)) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": stream base pointers must be 16-byte aligned");
    return PFMSCAN_OK;
}

static int mut_staged_check(pfmscan_ctx *ctx, const char *who)
{
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (ctx->staged_n < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no stream staged (call pfmscan_stage first)");
    if (!ctx->staged_codes && ctx->staged_n > 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": no codes are staged");
    return PFMSCAN_OK;
}

extern "C" {

int pfmscan_mutmap_dev(pfmscan_ctx *ctx, const pfmscan_motif *mo, const uint8_t *d_codes, int64_t n_pos, float *d_best,
                       int8_t *d_where, void *stream)
{
    if (int rc = mut_check(ctx, mo, d_codes, n_pos, "pfmscan_mutmap_dev")) return rc;
    if (n_pos > 0 && !d_best) return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_mutmap_dev: best is NULL");
    if (misaligned(d_best) || misaligned(d_where)) return fail(ctx, PFMSCAN_E_BADSHAPE, "pfmscan_mutmap_dev: output pointers must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MutArgs a{};
    a.codes = d_codes;
    a.n_pos = n_pos;
    a.table = mo->d_letters;
    a.m = mo->m;
    a.best = d_best;
    a.where = d_where;
    hipError_t e = launch_mutmap<false>(a, stream ? (hipStream_t)stream : ctx->stream);
    if (e != hipSuccess) return fail_hip(ctx, e, "k_mutmap");
    return PFMSCAN_OK;
}

int pfmscan_mutmap_staged(pfmscan_ctx *ctx, const pfmscan_motif *mo, float *best, int8_t *where)
{
    if (int rc = mut_staged_check(ctx, "pfmscan_mutmap_staged")) return rc;
    const int64_t n_pos = ctx->staged_n;
    if (int rc = mut_check(ctx, mo, (const uint8_t *)ctx->codes.p, n_pos, "pfmscan_mutmap_staged")) return rc;
    if (n_pos == 0) return PFMSCAN_OK;
    if (!best) return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_mutmap_staged: best is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = ensure(ctx, ctx->mut_best, (size_t)n_pos * 16))) return rc;
    if (where && (rc = ensure(ctx, ctx->mut_where, (size_t)n_pos * 4))) return rc;
    if ((rc = pfmscan_mutmap_dev(ctx, mo, (const uint8_t *)ctx->codes.p, n_pos, (float *)ctx->mut_best.p, where ? (int8_t *)ctx->mut_where.p : nullptr,
                                 ctx->stream)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(best, ctx->mut_best.p, (size_t)n_pos * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (where) HIP_TRY(ctx, hipMemcpyAsync(where, ctx->mut_where.p, (size_t)n_pos * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFMSCAN_OK;
}

int pfmscan_mutmap_events_dev(pfmscan_ctx *ctx, const pfmscan_motif *mo, const uint8_t *d_codes, int64_t n_pos, double thr,
                              int64_t capacity, int64_t *d_ev_key, float *d_ev_ref, float *d_ev_alt, uint64_t *d_ev_count, void *stream)
{
    if (int rc = mut_check(ctx, mo, d_codes, n_pos, "pfmscan_mutmap_events_dev")) return rc;
    if (std::isnan(thr)) return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_mutmap_events_dev: NaN threshold");
    if (capacity < 0 || !d_ev_count || (capacity > 0 && (!d_ev_key || !d_ev_ref || !d_ev_alt)))
        return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_mutmap_events_dev: bad event buffers");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MutArgs a{};
    a.codes = d_codes;
    a.n_pos = n_pos;
    a.table = mo->d_letters;
    a.m = mo->m;
    a.thr = thr;
    a.capacity = capacity;
    a.ev_key = d_ev_key;
    a.ev_ref = d_ev_ref;
    a.ev_alt = d_ev_alt;
    a.ev_count = reinterpret_cast<unsigned long long *>(d_ev_count);
    hipError_t e = launch_mutmap<true>(a, stream ? (hipStream_t)stream : ctx->stream);
    if (e != hipSuccess) return fail_hip(ctx, e, "k_mutmap (events)");
    return PFMSCAN_OK;
}

int pfmscan_mutmap_events_staged(pfmscan_ctx *ctx, const pfmscan_motif *mo, double thr, int64_t capacity, int64_t *ev_key,
                                 float *ev_ref, float *ev_alt, int64_t *n_events)
{
    if (int rc = mut_staged_check(ctx, "pfmscan_mutmap_events_staged")) return rc;
    if (!n_events) return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_mutmap_events_staged: n_events is NULL");
    const int64_t n_pos = ctx->staged_n;
    if (int rc = mut_check(ctx, mo, (const uint8_t *)ctx->codes.p, n_pos, "pfmscan_mutmap_events_staged")) return rc;
    if (std::isnan(thr)) return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_mutmap_events_staged: NaN threshold");
    if (capacity < 0 || (capacity > 0 && (!ev_key || !ev_ref || !ev_alt)))
        return fail(ctx, PFMSCAN_E_BADARG, "pfmscan_mutmap_events_staged: bad event buffers");
    *n_events = 0;
    if (n_pos == 0) return PFMSCAN_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t cap = (size_t)std::max<int64_t>(capacity, 1);
    if ((rc = ensure(ctx, ctx->mut_key, cap * 8))) return rc;
    if ((rc = ensure(ctx, ctx->mut_best, cap * 4))) return rc;
    if ((rc = ensure(ctx, ctx->mut_alt, cap * 4))) return rc;
    if ((rc = ensure(ctx, ctx->count, HIT_COUNTER_STRIDE * 8))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->count.p, 0, 8, ctx->stream));
    if ((rc = pfmscan_mutmap_events_dev(ctx, mo, (const uint8_t *)ctx->codes.p, n_pos, thr, capacity, (int64_t *)ctx->mut_key.p, (float *)ctx->mut_best.p,
                                        (float *)ctx->mut_alt.p, (uint64_t *)ctx->count.p, ctx->stream)))
        return rc;
    uint64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, ctx->count.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_events = (int64_t)total;
    if ((int64_t)total > capacity)
        return fail(ctx, PFMSCAN_E_CAPACITY, "pfmscan_mutmap_events_staged: " + std::to_string(total) + " events, capacity " + std::to_string(capacity));
    if (total == 0) return PFMSCAN_OK;
    std::vector<int64_t> key(total);
    std::vector<float> rf(total), al(total);
    HIP_TRY(ctx, hipMemcpyAsync(key.data(), ctx->mut_key.p, total * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rf.data(), ctx->mut_best.p, total * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(al.data(), ctx->mut_alt.p, total * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> order(total);                                   // keys are distinct: events are rare, sorted on the host
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key[x] < key[y]; });
    for (uint64_t i = 0; i < total; ++i) {
        ev_key[i] = key[order[i]];
        ev_ref[i] = rf[order[i]];
        ev_alt[i] = al[order[i]];
    }
    return PFMSCAN_OK;
}

int pfmscan_variants_dev(pfmscan_ctx *ctx, const double *letter_tables, int n_motifs, int m, const uint8_t *d_codes, int64_t n_pos,
                         const int64_t *d_var_pos, const uint8_t *d_var_alt, int64_t n_var, float *d_ref, float *d_alt,
                         int8_t *d_ref_where, int8_t *d_alt_where, void *stream)
{
    const char *who = "pfmscan_variants_dev";
    if (!ctx) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL ctx");
    if (!letter_tables) return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": no letters part (letter_tables is NULL)");
    if (n_motifs < 1) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": n_motifs must be positive");
    if (m < 1 || m > PFMSCAN_MAX_M)
        return fail(ctx, PFMSCAN_E_BADSHAPE, std::string(who) + ": width " + std::to_string(m) + " outside 1 .. PFMSCAN_MAX_M (" + std::to_string(PFMSCAN_MAX_M) + ")");
    if (n_pos < 0 || n_var < 0) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": negative size");
    if (n_pos > 0 && !d_codes) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": codes is NULL");
    if (n_var > 0 && (!d_var_pos || !d_var_alt || !d_ref || !d_alt)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL variant list or output");
    if (n_var == 0) return PFMSCAN_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const size_t bytes = (size_t)n_motifs * m * 8 * sizeof(double);
    if (int rc = ensure(ctx, ctx->mut_tab, bytes)) return rc;
    if (int rc = upload(ctx, ctx->mut_tab.p, letter_tables, bytes, st)) return rc;
    VarArgs a{};
    a.codes = d_codes;
    a.n_pos = n_pos;
    a.tables = (const double *)ctx->mut_tab.p;
    a.n_motifs = n_motifs;
    a.m = m;
    a.chunk = std::min(n_motifs, var_chunk(m));
    a.var_pos = d_var_pos;
    a.var_alt = d_var_alt;
    a.n_var = n_var;
    a.ref = d_ref;
    a.alt = d_alt;
    a.ref_where = d_ref_where;
    a.alt_where = d_alt_where;
    const int64_t gx = (n_var + VAR_PER_BLOCK - 1) / VAR_PER_BLOCK;
    const int gy = (n_motifs + a.chunk - 1) / a.chunk;
    if (gx > 0x7FFFFFFF || gy > 65535) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": too many variants or motifs for one call");
    hipLaunchKernelGGL(k_variants, dim3((unsigned)gx, (unsigned)gy), dim3(BLOCK), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(ctx, e, "k_variants");
    return PFMSCAN_OK;
}

int pfmscan_variants_staged(pfmscan_ctx *ctx, const double *letter_tables, int n_motifs, int m, const int64_t *var_pos,
                            const uint8_t *var_alt, int64_t n_var, float *ref, float *alt, int8_t *ref_where, int8_t *alt_where)
{
    const char *who = "pfmscan_variants_staged";
    if (int rc = mut_staged_check(ctx, who)) return rc;
    if (n_var < 0 || n_motifs < 1) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": bad sizes");
    if (n_var > 0 && (!var_pos || !var_alt || !ref || !alt)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NULL variant list or output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)n_var * n_motifs;
    int rc;
    if ((rc = ensure(ctx, ctx->mut_key, std::max<size_t>((size_t)n_var * 8, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->mut_valt, std::max<size_t>((size_t)n_var, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->mut_best, std::max<size_t>(cells * 4, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->mut_alt, std::max<size_t>(cells * 4, 16)))) return rc;
    if ((rc = ensure(ctx, ctx->mut_where, std::max<size_t>(cells * 2, 16)))) return rc;
    if (n_var > 0) {
        if ((rc = upload(ctx, ctx->mut_key.p, var_pos, (size_t)n_var * 8, ctx->stream))) return rc;
        if ((rc = upload(ctx, ctx->mut_valt.p, var_alt, (size_t)n_var, ctx->stream))) return rc;
    }
    int8_t *d_rw = (int8_t *)ctx->mut_where.p, *d_aw = d_rw + cells;
    if ((rc = pfmscan_variants_dev(ctx, letter_tables, n_motifs, m, (const uint8_t *)ctx->codes.p, ctx->staged_n, (const int64_t *)ctx->mut_key.p,
                                   (const uint8_t *)ctx->mut_valt.p, n_var, (float *)ctx->mut_best.p, (float *)ctx->mut_alt.p,
                                   ref_where ? d_rw : nullptr, alt_where ? d_aw : nullptr, ctx->stream)))
        return rc;
    if (n_var > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(ref, ctx->mut_best.p, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(alt, ctx->mut_alt.p, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (ref_where) HIP_TRY(ctx, hipMemcpyAsync(ref_where, d_rw, cells, hipMemcpyDeviceToHost, ctx->stream));
        if (alt_where) HIP_TRY(ctx, hipMemcpyAsync(alt_where, d_aw, cells, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PFMSCAN_OK;
}

}  // extern "C"
