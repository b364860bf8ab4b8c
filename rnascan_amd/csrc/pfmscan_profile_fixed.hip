// pfmscan_profile_fixed.hip -- k_profile (codes + averaged-structure profile: all scores and the fused hits pass) with the
// PFM width as a COMPILE-TIME constant.  Same tile, same operation order and therefore the same bits as the width-generic
// kernel in pfmscan_kernels.hip (rnascan.py:302-307 for the structure rows, _pwm.c:34-68 for the letters); what the
// constant buys is VALU issue slots, the unit the headline kernel is shortest of once its bytes are moving:
//   * the row loop is straight-line code: no round counter, no per-round advance of the V letter addresses and of the row
//     pointer (27 VALU instructions per wave and tile), every LDS offset an immediate of its ds_read;
//   * the slide-in after the LAST row -- a row no window of the thread uses -- is not loaded or converted (7 + 4);
//   * the stager walks the tile's pieces on the scalar unit and leaves the codes as offsets into the letter table, so a letter
//     look-up needs no address arithmetic (27 + 32); the interior tile's output path addresses LDS and memory by one lane
//     register + immediates (profiles/fixed_isa/isa_count.md: 708 -> 630 VALU instructions per wave and tile at w = 12).
// Widths without an instantiation (below 9 rows by measurement, above 18) run the generic kernel (launch_profile_fixed says no).
#include <cstdlib>
#include "pfmscan_profile.hpp"

namespace pfmscan {

// The letter look-up of a position is one ds_read_b64 at  table + j * 64 + (code & 7) * 8.  The stager below leaves
// (code & 7) * 8 in the tile's code bytes instead of the code (two VALU instructions per DWORD of codes while it is in
// registers anyway), so a thread's ds_read_u8 returns the low part of the address as it is.  Where the kernel has no static
// LDS (ABS: the all-scores instantiations; the launcher checks it) the dynamic region starts at LDS address 0, the table's
// place in it is a constant and goes into the ds_read's immediate with j * 64: no address arithmetic at all.  Elsewhere
// (the hits instantiations: emit_hits_block owns a static word) the table's address is added once per position.
__device__ __forceinline__ uint32_t code_offsets4(uint32_t codes4) { return (codes4 & 0x07070707u) << 3; }

// dma_issue16 with the global address as wave-uniform base (SGPR pair) + 32-bit lane offset: walking the pieces of a tile is
// scalar arithmetic (it was a 64-bit VALU add, a VALU add and a compare per piece: 27 per wave and tile at float32 rows)
__device__ __forceinline__ void dma_issue16_sbase(const void *gbase, uint32_t lane_off, uint32_t lds_base)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane_off), "s"(gbase), "s"(lds_base)
                 : "memory");
}

// true iff every position in [0, end) lies inside the stream, decided on the scalar unit: a 64-bit signed compare is a VALU
// instruction, a subtraction and the sign of its high word are not (the empty asm keeps hipcc from folding the two back
// into the compare)
__device__ __forceinline__ bool ends_inside(int64_t end, int64_t n_pos)
{
    int32_t hi = (int32_t)((uint64_t)(n_pos - end) >> 32);
    asm("" : "+s"(hi));
    return hi >= 0;
}

// stage_tile (pfmscan_profile.hpp) for the fixed-width kernel: the same bytes into the same places, the interior tile's rows by
// LDS-DMA off a scalar base, the codes through registers and stored as table offsets (code_offsets4)
template <int V, int MW, bool HAS_SEQ, typename PROF_T>
__device__ __forceinline__ void stage_tile_fixed(const ScanArgs &a, int64_t tile0, unsigned char *buf)
{
    using L = ProfileLayout<V, PROF_T>;
    constexpr int prof_bytes = L::prof_bytes(MW), code_bytes = L::code_bytes(MW);
    constexpr int npiece = prof_bytes >> 10;
    constexpr int pneed = (L::TILE + MW) * 7 * (int)sizeof(PROF_T), cneed = L::TILE + MW;     // see stage_tile
    const int tid = threadIdx.x;
    const int64_t n_pos = a.n_pos;
    const int64_t total_bytes = n_pos * 7 * (int64_t)sizeof(PROF_T);
    const int64_t g0 = tile0 * 7 * (int64_t)sizeof(PROF_T);
    const unsigned char *gsrc = reinterpret_cast<const unsigned char *>(a.profile) + g0;
    const bool interior = ends_inside(g0 + prof_bytes, total_bytes) && (!HAS_SEQ || ends_inside(tile0 + code_bytes, n_pos));
    if (interior) {
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const uint32_t lane16 = (uint32_t)(tid & 63) << 4;
        const uint32_t base = lds_addr(buf);
        for (int pc = wave; pc < npiece; pc += BLOCK / 64) {      // pc is wave-uniform: only the last piece pays the lane test
            if (pc + 1 < npiece)
                dma_issue16_sbase(gsrc + ((size_t)pc << 10), lane16, base + ((uint32_t)pc << 10));
            else if (a.dma_whole || ((npiece - 1) << 10) + (int)lane16 < pneed)
                dma_issue16_sbase(gsrc + ((size_t)(npiece - 1) << 10), lane16, base + ((uint32_t)(npiece - 1) << 10));
        }
        if (HAS_SEQ) {
            static_assert((cneed + 15) / 16 <= BLOCK, "one 16-byte vector of codes per thread");
            if (tid < (cneed + 15) / 16) {
                u32x4 c = reinterpret_cast<const u32x4 *>(a.codes + tile0)[tid];
                c.x = code_offsets4(c.x), c.y = code_offsets4(c.y), c.z = code_offsets4(c.z), c.w = code_offsets4(c.w);
                reinterpret_cast<u32x4 *>(buf + prof_bytes)[tid] = c;
            }
        }
    } else {
        const int ndw = prof_bytes >> 2;
        const int64_t valid_dw = (total_bytes - g0) >> 2;
        for (int c = tid; c < ndw; c += BLOCK)
            reinterpret_cast<uint32_t *>(buf)[c] = (c < valid_dw) ? reinterpret_cast<const uint32_t *>(gsrc)[c] : 0u;
        if (HAS_SEQ) {
            const int ncw = code_bytes >> 2;
            for (int c = tid; c < ncw; c += BLOCK)
                reinterpret_cast<uint32_t *>(buf + prof_bytes)[c] = code_offsets4(load_codes4(a.codes, tile0 + 4 * (int64_t)c, n_pos));
        }
    }
}

// LDS address of the letter whose staged byte is `off8` in row 0 of the table at `tbase`.  FOLD: plain arithmetic on a constant,
// which hipcc moves into the ds_read's immediate.  Otherwise ONE v_add_u32 whose result the compiler cannot look into: left to
// itself it re-associates tbase + j * 64 into a scalar and adds THAT at every look-up (5 adds per step instead of one)
template <bool FOLD>
__device__ __forceinline__ uint32_t letter_addr(uint32_t off8, uint32_t tbase)
{
    if (FOLD) return off8 + tbase;
    uint32_t a;
    asm("v_add_u32 %0, %1, %2" : "=v"(a) : "s"(tbase), "v"(off8));
    return a;
}

template <int V, bool HAS_SEQ>
__device__ __forceinline__ void pin_sums(double (&st)[V], double (&sq)[V])
{
    static_assert(V == 5, "one operand list per V");
    if (HAS_SEQ)
        asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(st[4]), "+v"(sq[0]), "+v"(sq[1]), "+v"(sq[2]), "+v"(sq[3]), "+v"(sq[4])::"memory");
    else
        asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(st[4])::"memory");
}

template <int V, int MW, bool HAS_SEQ, typename PROF_T, bool FINITE, bool ABS>
__device__ __forceinline__ void compute_tile_fixed(const PROF_T *prof_lds, const unsigned char *code_lds, const char *tseq_lds,
                                                   const double *__restrict__ pssm, int la, double (&acc_st)[V], double (&acc_sq)[V])
{
    double rows[V][7];
    using L = ProfileLayout<V, PROF_T>;
    uint32_t sadr[V];                // LDS address of this slot's letter in table row 0 (FOLD: less the table's place); row j is the immediate offset j * 64
    // FOLD: the table's place is a constant AND fits the 16-bit ds_read offset together with the row (float32 rows: 38 912 + 17 * 64
    // + 56; float64 rows put the table at 75 776) -- the staged byte IS the address register.  Otherwise the table's address is
    // added once per position by letter_addr, whose result is opaque, so that j * 64 stays the read's immediate
    constexpr uint32_t tplace = (uint32_t)(L::prof_bytes(MW) + L::code_bytes(MW));
    constexpr bool FOLD = ABS && tplace + (MW - 1) * 64 + 56 <= 65535;
    const uint32_t tbase = ABS ? tplace : lds_addr(tseq_lds);
    const PROF_T *mine = prof_lds + la * 7;           // the thread's first row: every later row is an immediate offset
    const unsigned char *cmine = code_lds + la;
#pragma unroll
    for (int s = 0; s < V; ++s) {
#pragma unroll
        for (int k = 0; k < 7; ++k) rows[s][k] = (double)mine[s * 7 + k];
        sadr[s] = HAS_SEQ ? letter_addr<FOLD>(cmine[s], tbase) : 0u;          // the staged byte is (code & 7) * 8
        acc_st[s] = 0.0;
        acc_sq[s] = 0.0;
    }
    const __attribute__((address_space(4))) double *ptab = (const __attribute__((address_space(4))) double *)pssm;
    double Pn[7];                                     // PSSM row of the NEXT step (SGPRs), requested one step ahead
#pragma unroll
    for (int k = 0; k < 7; ++k) Pn[k] = ptab[k];
#pragma unroll
    for (int j = 0; j < MW; ++j) {
        const int u = j % V;
        double P[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) P[k] = Pn[k];
        // (a) everything the step reads, requested before its arithmetic: the V table values, the row that slides in at the
        //     end (as stored), its letter, and the next PSSM row -- their latency runs under the 35 FMAs below
        double tv[V];
        PROF_T nr[7];
        uint32_t ncode = 0;
        if (HAS_SEQ) {
#pragma unroll
            for (int v = 0; v < V; ++v) tv[v] = *(const __attribute__((address_space(3))) double *)(uintptr_t)(sadr[(u + v) % V] + j * 64);
        }
        if (j + 1 < MW) {                             // the slide-in after the last row has no reader
#pragma unroll
            for (int k = 0; k < 7; ++k) nr[k] = mine[(j + V) * 7 + k];
            if (HAS_SEQ) ncode = cmine[j + V];
#pragma unroll
            for (int k = 0; k < 7; ++k) Pn[k] = ptab[(j + 1) * 7 + k];
        }
        __builtin_amdgcn_sched_barrier(0);
        // (b) the arithmetic, in the reference's order per window
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int slot = (u + v) % V;             // holds stream position la + v + j
            if (FINITE) {
                double sacc = acc_st[v];
#pragma unroll
                for (int k = 0; k < 7; ++k) sacc = fma(rows[slot][k], P[k], sacc);
                acc_st[v] = sacc;
            } else {
                double d = rows[slot][0] * P[0];
#pragma unroll
                for (int k = 1; k < 7; ++k) d = fma(rows[slot][k], P[k], d);
                acc_st[v] += nan_to_num(d);
            }
            if (HAS_SEQ) acc_sq[v] += tv[v];
        }
        // (c) slot u is dead: position la + j + V slides in
        if (j + 1 < MW) {
#pragma unroll
            for (int k = 0; k < 7; ++k) rows[u][k] = (double)nr[k];
            if (HAS_SEQ) sadr[u] = letter_addr<FOLD>(ncode, tbase);
        }
        // One row step stays one step.  The unrolled loop is a single basic block, and left alone the instruction selector
        // linearises it with the sums of later steps deferred and their operands (rows, table values) held -- 230 VGPRs spilled
        // at w = 12.  The empty asm takes every running sum as an in/out operand (no instruction is emitted), which pins the
        // step's FMAs and adds in front of it; the memory clobber does the same for the LDS reads, the fence below for the
        // machine scheduler.
        pin_sums<V, HAS_SEQ>(acc_st, acc_sq);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (FINITE) {
        // one branch for the thread's V windows (the tests are V compares either way; the slow path's set-up stays behind it)
        bool any = false;
#pragma unroll
        for (int v = 0; v < V; ++v) any = any || !(fabs(acc_st[v]) <= DBL_MAX);
        if (any) {
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (!(fabs(acc_st[v]) <= DBL_MAX)) acc_st[v] = struct_window_slow(prof_lds, la + v, pssm, MW);
        }
    }
}

// emit_tile_wave (pfmscan_profile.hpp) for a tile whose every output vector lies inside the stream, the width a constant:
// the same staging in the wave's own part of the tile buffer, the same 16-byte stores.  Every LDS address is one per-lane
// register (lane * 40, lane * 20, lane * 16 off the wave's scalar base) + an immediate, every global address the wave's
// scalar base + lane * 16 + an immediate.
template <int V, int MW, bool HAS_SEQ, typename PROF_T>
__device__ __forceinline__ void emit_tile_wave_inside(const ScanArgs &a, int64_t tile0, const double (&acc_st)[V],
                                                      const double (&acc_sq)[V], unsigned char *tile_buf)
{
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) float lds_f32;
    typedef __attribute__((address_space(3))) const f32x4 lds_f32x4;
    typedef __attribute__((address_space(3))) const f64x2 lds_f64x2;
    constexpr int WN = 64 * V;                      // windows per wave
    const uint32_t lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t band = lds_addr(tile_buf) + (uint32_t)(((wave * WN + MW - 1) * 7 * (int)sizeof(PROF_T) + 15) & ~15);
    const uint32_t st_w = band + lane * (V * 8), sq_w = band + WN * 8 + lane * (V * 4);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        *(lds_f64 *)(uintptr_t)(st_w + v * 8) = acc_st[v];
        if (HAS_SEQ) *(lds_f32 *)(uintptr_t)(sq_w + v * 4) = (float)acc_sq[v];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t w0 = tile0 + (int64_t)wave * WN;  // first window of the wave's band
    const uint32_t rd = band + lane * 16, off = lane * 16;
    if (HAS_SEQ && a.out_seq) {
        char *dst = reinterpret_cast<char *>(a.out_seq + w0);
#pragma unroll
        for (int c0 = 0; c0 < WN / 4; c0 += 64)
            if (c0 + 64 <= WN / 4 || lane < (uint32_t)(WN / 4 - c0))
                __builtin_nontemporal_store(*(lds_f32x4 *)(uintptr_t)(rd + WN * 8 + c0 * 16), reinterpret_cast<f32x4 *>(dst + off + c0 * 16));
    }
    if (a.out_struct) {
        char *dst = reinterpret_cast<char *>(a.out_struct + w0);
#pragma unroll
        for (int c0 = 0; c0 < WN / 2; c0 += 64)
            if (c0 + 64 <= WN / 2 || lane < (uint32_t)(WN / 2 - c0))
                __builtin_nontemporal_store(*(lds_f64x2 *)(uintptr_t)(rd + c0 * 16), reinterpret_cast<f64x2 *>(dst + off + c0 * 16));
    }
}

template <int V, int MW, bool HAS_SEQ, typename PROF_T, bool FINITE, bool HITS, bool SUM>
__device__ __forceinline__ void profile_fixed_body(const ScanArgs &a)
{
    using L = ProfileLayout<V, PROF_T>;
    extern __shared__ __align__(16) unsigned char smem[];
    const int64_t tile0 = (int64_t)blockIdx.x * L::TILE;
    constexpr int prof_bytes = L::prof_bytes(MW);
    char *tseq_lds = reinterpret_cast<char *>(smem + prof_bytes + (HAS_SEQ ? L::code_bytes(MW) : 0));
    if (a.prio) __builtin_amdgcn_s_setprio(3);        // see k_profile
    stage_tile_fixed<V, MW, HAS_SEQ, PROF_T>(a, tile0, smem);
    if (HAS_SEQ)
        for (int i = threadIdx.x; i < MW * 8; i += BLOCK) reinterpret_cast<double *>(tseq_lds)[i] = a.letter_table[i];
    if (a.prio) __builtin_amdgcn_s_setprio(0);
    dma_wait_all();
    __syncthreads();
    const int la = threadIdx.x * V;
    double acc_st[V], acc_sq[V];
    compute_tile_fixed<V, MW, HAS_SEQ, PROF_T, FINITE, !HITS>(reinterpret_cast<const PROF_T *>(smem), smem + prof_bytes, tseq_lds, a.struct_pssm,
                                                              la, acc_st, acc_sq);
    if (HITS) {
        settle_near<V, PROF_T>(a, reinterpret_cast<const PROF_T *>(smem), la, acc_st);
        // the fused combined filter: seq > thr && struct > thr (SUM: && printed sum > thr_sum)
        emit_tile_hits<V, HAS_SEQ, SUM, PROF_T>(a, tile0, la, acc_st, acc_sq, reinterpret_cast<const PROF_T *>(smem));
    }
    else if (ends_inside(tile0 + V * BLOCK + MW, a.n_pos))                    // workgroup-uniform: false only for the last tile(s) of the stream
        emit_tile_wave_inside<V, MW, HAS_SEQ, PROF_T>(a, tile0, acc_st, acc_sq, smem);
    else
        emit_tile_wave<V, HAS_SEQ, PROF_T>(a, tile0, la, acc_st, acc_sq, smem, MW);
}

template <int V, int MW, bool HAS_SEQ, typename PROF_T, bool FINITE, bool HITS>
__global__ __launch_bounds__(BLOCK, 4) void k_profile_fixed(const ScanArgs a)
{
    profile_fixed_body<V, MW, HAS_SEQ, PROF_T, FINITE, HITS, false>(a);
}

// the fused combined hits pass with the third predicate  LogOdds.SeqStruct > a.thr_sum  (pfmscan_exact.hpp)
template <int V, int MW, typename PROF_T, bool FINITE>
__global__ __launch_bounds__(BLOCK, 4) void k_profile_fixed_sum(const ScanArgs a)
{
    profile_fixed_body<V, MW, true, PROF_T, FINITE, true, true>(a);
}

template <int MW, typename PROF_T, bool FINITE>
static hipError_t launch_fixed_sum_inst(const ScanArgs &a, hipStream_t stream)
{
    constexpr int V = PROFILE_V;
    using L = ProfileLayout<V, PROF_T>;
    const unsigned grid = (unsigned)((a.n_pos + L::TILE - 1) / L::TILE);
    const int lds = L::total(MW, true, 1);
    auto kern = k_profile_fixed_sum<V, MW, PROF_T, FINITE>;
    static std::atomic<uint64_t> configured{0};     // per instantiation, one bit per device
    hipError_t e = allow_full_lds(reinterpret_cast<const void *>(kern), configured);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), lds, stream, a);
    return hipGetLastError();
}

template <int MW>
static hipError_t launch_fixed_sum_width(const ScanArgs &a, hipStream_t stream)
{
    const bool fin = a.struct_finite != 0;
    if (a.profile_dtype == PFMSCAN_PROFILE_F64)
        return fin ? launch_fixed_sum_inst<MW, double, true>(a, stream) : launch_fixed_sum_inst<MW, double, false>(a, stream);
    return fin ? launch_fixed_sum_inst<MW, float, true>(a, stream) : launch_fixed_sum_inst<MW, float, false>(a, stream);
}

template <int MW, bool HAS_SEQ, typename PROF_T, bool FINITE, bool HITS>
static hipError_t launch_fixed_inst(const ScanArgs &a, hipStream_t stream, bool *taken)
{
    constexpr int V = PROFILE_V;
    using L = ProfileLayout<V, PROF_T>;
    const unsigned grid = (unsigned)((a.n_pos + L::TILE - 1) / L::TILE);
    const int lds = L::total(MW, HAS_SEQ, 1);
    auto kern = k_profile_fixed<V, MW, HAS_SEQ, PROF_T, FINITE, HITS>;
    static std::atomic<uint64_t> configured{0};     // per instantiation, one bit per device
    hipError_t e = allow_full_lds(reinterpret_cast<const void *>(kern), configured);
    if (e != hipSuccess) return e;
    if (!HITS) {
        // the all-scores instantiations address the letter table by its place in the dynamic region (compute_tile_fixed, ABS):
        // right as long as the kernel has no static LDS in front of it.  If it ever has, the generic kernel takes the scan
        static std::atomic<int> static_lds{-1};
        int sl = static_lds.load(std::memory_order_relaxed);
        if (sl < 0) {
            hipFuncAttributes fa;
            e = hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(kern));
            if (e != hipSuccess) return e;
            sl = (int)fa.sharedSizeBytes;
            static_lds.store(sl, std::memory_order_relaxed);
        }
        if (sl != 0) {
            *taken = false;
            return hipSuccess;
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), lds, stream, a);
    return hipGetLastError();
}

template <int MW, bool HITS>
static hipError_t launch_fixed_width(const ScanArgs &a, hipStream_t stream, bool *taken)
{
    const bool has_seq = a.letter_table != nullptr, fin = a.struct_finite != 0;
    if (a.profile_dtype == PFMSCAN_PROFILE_F64) {
        if (has_seq) return fin ? launch_fixed_inst<MW, true, double, true, HITS>(a, stream, taken) : launch_fixed_inst<MW, true, double, false, HITS>(a, stream, taken);
        return fin ? launch_fixed_inst<MW, false, double, true, HITS>(a, stream, taken) : launch_fixed_inst<MW, false, double, false, HITS>(a, stream, taken);
    }
    if (has_seq) return fin ? launch_fixed_inst<MW, true, float, true, HITS>(a, stream, taken) : launch_fixed_inst<MW, true, float, false, HITS>(a, stream, taken);
    return fin ? launch_fixed_inst<MW, false, float, true, HITS>(a, stream, taken) : launch_fixed_inst<MW, false, float, false, HITS>(a, stream, taken);
}

// true when a fixed-width instantiation took the scan (all scores, or the fused hits pass), result in *err; false: the caller
// runs the generic kernel
bool launch_profile_fixed(const ScanArgs &a, hipStream_t stream, hipError_t *err)
{
    const bool off = std::getenv("PFMSCAN_PROFILE_GENERIC") != nullptr;      // tests and A/B runs: the width-generic kernel
    if (off || !a.struct_pssm || !a.profile || a.out_letters_f64) return false;
    // C3 with placed arrays, generic / fixed in ms (tools/ab_fixed.sh, three interleaved pairs each, profiles/r4/NOTES.md):
    // w = 6: 2.00 / 1.99, 8: 1.960 / 1.974, 9: 1.990 / 1.976, 10: 2.038 / 1.966, 11: 2.107 / 1.993, 12: 2.188 / 2.052,
    // 16: 2.538 / 2.328, 18: 2.707 / 2.475 -- below nine rows the generic loop's two full rounds of five cost nothing extra
    int min_w = 9;
    if (const char *v = std::getenv("PFMSCAN_PROFILE_FIXED_MIN")) min_w = std::atoi(v);
    if (a.m < min_w) return false;
    bool taken = true;          // an instantiation may still decline (launch_fixed_inst)
    if (sum_active(a)) {        // joint threshold: the *_sum instantiation of the width (both parts present: pfmscan_hits_sum_* checks)
        if (!a.letter_table) return false;
        switch (a.m) {
#define FIXED_WIDTH(W) case W: *err = launch_fixed_sum_width<W>(a, stream); return true;
        FIXED_WIDTH(4) FIXED_WIDTH(5) FIXED_WIDTH(6) FIXED_WIDTH(7) FIXED_WIDTH(8) FIXED_WIDTH(9) FIXED_WIDTH(10) FIXED_WIDTH(11)
        FIXED_WIDTH(12) FIXED_WIDTH(13) FIXED_WIDTH(14) FIXED_WIDTH(15) FIXED_WIDTH(16) FIXED_WIDTH(17) FIXED_WIDTH(18)
#undef FIXED_WIDTH
        default: return false;
        }
    }
    switch (a.m) {
#define FIXED_WIDTH(W) case W: *err = a.hits ? launch_fixed_width<W, true>(a, stream, &taken) : launch_fixed_width<W, false>(a, stream, &taken); return taken;
    FIXED_WIDTH(4) FIXED_WIDTH(5) FIXED_WIDTH(6) FIXED_WIDTH(7) FIXED_WIDTH(8) FIXED_WIDTH(9) FIXED_WIDTH(10) FIXED_WIDTH(11)
    FIXED_WIDTH(12) FIXED_WIDTH(13) FIXED_WIDTH(14) FIXED_WIDTH(15) FIXED_WIDTH(16) FIXED_WIDTH(17) FIXED_WIDTH(18)
#undef FIXED_WIDTH
    default: return false;
    }
}

}  // namespace pfmscan
