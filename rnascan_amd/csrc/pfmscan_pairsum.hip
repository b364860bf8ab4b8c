// pfmscan_pairsum.hip -- the joint threshold on the printed LogOdds.SeqStruct of the two-FASTA mode
// (`rnascan -p .. -q .. seqs.fa structs.fa --min-seqstruct T`; rnascan.py:273, :416-434; pfmscan_hits_pair_sum_*).
//
//  k_pair_sum_dense   BOTH exact letter sums of EVERY window in one pass, then the whole predicate
//                         f > thr_seq  and  st > thr_struct  and  (double) round3(f) + round3d(st) > thr_sum
//              (pair_sum_passes, pfmscan_exact.hpp).  The exact fallback of thr_seq = -inf: widths above 32 (up to
//              PFMSCAN_MAX_WIDTH), a switched-off prefilter, a predicted survivor rate above 1/32.  No list of candidates,
//              no score array, nothing leaves the device but the hits.  (With a finite thr_seq the sequence letters select
//              first: k_letters_cred<.., PAIR, SUM> in one launch; where they decline, k_pair_cred_sum if the joint credits
//              are sparse, else a letters pass and k_letters_at<SUM>.)
//
//              A workgroup parks the codes of its 2048 windows (+ m bytes of look-ahead) of both streams in LDS once.  The
//              two tables pass through LDS in slabs of 64 rows (m <= 64: one slab).  A thread owns 8 consecutive windows:
//              the 8 code bytes they meet in row j are ONE 64-bit register that slides by a byte per row (one ds_read_u8
//              per row and stream), every look-up of a row hits the same 64-byte table row (at most 8 addresses, no bank
//              conflict), and the sums run row after row in fp64 -- the order of _pwm.c:34-68 / matrix.py:25-43, so every
//              bit of f and st is the reference's.  Foreign letters and positions past the stream read the NaN column.
//              Hits leave through emit_hits_block: one returning atomic per workgroup that has any.
//
//  k_pair_cred_sum  the integer prefilter of the joint threshold, for PFMs up to width 32: ONE 16-bit credit sum per window
//              takes contributions from BOTH code streams.  Both tables are single-letter credit tables in the layout of
//              k_letters_cred8 (one entry per code = that code's credit for EVERY row, two rows per dword), quantised with
//              ONE common quantum as one table of 2 m rows (build_pair_credits: build_credits over the rows of both
//              tables), the joint threshold -- thr_sum minus the margin of the cheap test -- folded into row 0 of the
//              sequence side.  The two streams are parked in LDS as ONE byte per position (sequence code | structure code
//              << 3), so the kernel holds the code buffers of k_letters_cred8; a lane owns 16 consecutive windows and reads
//              each table once per position of its band; bit 15 of a sum clear <=> the window's printed sum cannot pass.
//              Survivors wait in SurvivorQueue and get, 64 at a time, both exact letter sums from global memory (L2),
//              sequential fp64, the float32 cast on the sequence side, then the whole predicate; hits go through
//              WaveHitQueue (one returning atomic per flush).  No scratch, no float atomics.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>
#include "pfmscan_device.hpp"

namespace pfmscan {

constexpr int PSD_W = 8;                               // windows per thread
constexpr int PSD_TILE = BLOCK * PSD_W;                // windows per workgroup
constexpr int PSD_SLAB = 64;                           // table rows in LDS at a time
constexpr int PSD_CODES = PSD_TILE + PFMSCAN_MAX_WIDTH + 16;    // bytes 0 .. PSD_TILE + m - 1 of the tile, padded to dwords

__global__ __launch_bounds__(BLOCK) void k_pair_sum_dense(const ScanArgs a)
{
    __shared__ __align__(16) double t1[PSD_SLAB * 8], t2[PSD_SLAB * 8];
    __shared__ __align__(16) uint8_t cb1[PSD_CODES], cb2[PSD_CODES];
    const int m = a.m;
    const int64_t n_pos = a.n_pos;
    const int64_t tile0 = (int64_t)blockIdx.x * PSD_TILE;
    const int ndw = (PSD_TILE + m + 3) >> 2;           // <= (PSD_TILE + PFMSCAN_MAX_WIDTH + 3) / 4 dwords: inside cb1 / cb2
    for (int i = threadIdx.x; i < ndw; i += BLOCK) {
        reinterpret_cast<uint32_t *>(cb1)[i] = load_codes4(a.codes, tile0 + 4 * (int64_t)i, n_pos);
        reinterpret_cast<uint32_t *>(cb2)[i] = load_codes4(a.codes2, tile0 + 4 * (int64_t)i, n_pos);
    }
    const int off = threadIdx.x * PSD_W;
    double s1[PSD_W], s2[PSD_W];
#pragma unroll
    for (int v = 0; v < PSD_W; ++v) s1[v] = s2[v] = 0.0;
    uint64_t w1 = 0, w2 = 0;                           // byte v = the code window v meets in the current row
    for (int j0 = 0; j0 < m; j0 += PSD_SLAB) {         // workgroup-uniform
        const int rows = min(PSD_SLAB, m - j0);
        __syncthreads();                               // the codes are parked / the previous slab has been read
        for (int i = threadIdx.x; i < rows * 8; i += BLOCK) {
            t1[i] = a.letter_table[j0 * 8 + i];
            t2[i] = a.letter_table2[j0 * 8 + i];
        }
        __syncthreads();
        if (j0 == 0) {
            w1 = *reinterpret_cast<const uint64_t *>(cb1 + off);
            w2 = *reinterpret_cast<const uint64_t *>(cb2 + off);
        }
        for (int j = 0; j < rows; ++j) {
            const double *r1 = t1 + j * 8, *r2 = t2 + j * 8;
            static_for<0, PSD_W>([&](auto vc) __attribute__((always_inline)) {
                constexpr int v = decltype(vc)::value;
                s1[v] += r1[(uint32_t)(w1 >> (8 * v)) & 7u];
                s2[v] += r2[(uint32_t)(w2 >> (8 * v)) & 7u];
            });
            // the byte that enters: position off + (j0 + j) + 8 <= PSD_TILE + m - 1, parked above
            w1 = (w1 >> 8) | ((uint64_t)cb1[off + j0 + j + PSD_W] << 56);
            w2 = (w2 >> 8) | ((uint64_t)cb2[off + j0 + j + PSD_W] << 56);
        }
    }
    uint32_t mask = 0;
    const int64_t p0 = tile0 + off;
    float f[PSD_W];
    static_for<0, PSD_W>([&](auto vc) __attribute__((always_inline)) {
        constexpr int v = decltype(vc)::value;
        f[v] = (float)s1[v];
        if (p0 + v < n_pos && (double)f[v] > a.thr_seq && s2[v] > a.thr_struct && pair_sum_passes(f[v], s2[v], a.thr_sum, a.sum_margin0))
            mask |= 1u << v;
    });
    // compile-time selects: neither f[] nor s2[] is ever indexed at run time
    auto pick_f = [&](int i) { float r = f[0]; static_for<1, PSD_W>([&](auto vc) __attribute__((always_inline)) { if (i == decltype(vc)::value) r = f[decltype(vc)::value]; }); return r; };
    auto pick_s = [&](int i) { double r = s2[0]; static_for<1, PSD_W>([&](auto vc) __attribute__((always_inline)) { if (i == decltype(vc)::value) r = s2[decltype(vc)::value]; }); return r; };
    emit_hits_block<PSD_W>(mask, [&](int i) { return p0 + i; }, pick_f, pick_s, a);
}

// ---------------------------------------------------------------------------
// k_pair_cred_sum
// ---------------------------------------------------------------------------
struct PairCredTable {
    uint32_t d[2][8][16];                              // [stream][code][row pair k] = credit of row 2k | credit of row 2k+1 << 16
};
constexpr int PCS_QCAP = 64;                           // hits a wave can park (16 bytes each): joint hits are rare

template <int NJ>
__global__ __launch_bounds__(BLOCK) void k_pair_cred_sum(const ScanArgs a, const PairCredTable ct)
{
    constexpr int W = 16;                              // windows per lane = one round per tile
    constexpr int LET_TILE = BLOCK * W;
    constexpr int NPOS = W + 2 * NJ - 1;               // positions a lane looks up: q = 0 .. W + 2 NJ - 2
    constexpr int NWD = (NPOS + 3) / 4;                // code dwords holding bytes 0 .. NPOS - 1
    constexpr int ESTR = NJ <= 2 ? 8 : (NJ <= 4 ? 16 : (NJ <= 8 ? 32 : 80));      // entry stride in bytes, as k_letters_cred8
    constexpr int PSH = NJ <= 2 ? 3 : (NJ <= 4 ? 4 : (NJ <= 8 ? 5 : 4));
    constexpr int EDW = ESTR / 4;
    constexpr int TROWS = 2 * NJ;                      // rows of the exact letter tables (rows m .. are zeros)
    constexpr int NRAW = (2 * NJ + 3) / 4 + 1;         // aligned code dwords that hold a window's 2 NJ letters at any p & 3
    constexpr int NWAVE = BLOCK / 64;
    static_assert(NPOS - W < CODE_HALO - 4, "look-ahead exceeds the code halo");
    __shared__ __align__(16) double tbl[2][TROWS * 8];
    __shared__ __align__(16) uint32_t ctab[2][8 * EDW];
    __shared__ __align__(16) uint8_t cbuf[2][LET_TILE + CODE_HALO];         // byte = sequence code & 7 | (structure code & 7) << 3
    __shared__ HitQueueLds<float, PCS_QCAP, true> hq_lds;
    __shared__ uint32_t sv_pos[NWAVE][SV_CAP];
    const int m = a.m;
    const int64_t n_pos = a.n_pos;
    const int ntile = a.tiles_per_block;
    const int64_t first = (int64_t)blockIdx.x * ntile * LET_TILE;
    if (first >= n_pos) return;                        // whole workgroup

    CodeStage<LET_TILE> cs, cs2;
    auto fetch2 = [&](int64_t t0) {
        cs.fetch(a.codes, t0, n_pos);
        cs2.fetch(a.codes2, t0, n_pos);
    };
    auto park2 = [&](uint8_t *dst) {
#pragma unroll
        for (int k = 0; k < CodeStage<LET_TILE>::PER; ++k) cs.r[k] = (cs.r[k] & 0x07070707u) | ((cs2.r[k] & 0x07070707u) << 3);
        cs.park(dst);
    };
    fetch2(first);
    for (int i = threadIdx.x; i < TROWS * 8; i += BLOCK) {
        tbl[0][i] = i < m * 8 ? a.letter_table[i] : 0.0;
        tbl[1][i] = i < m * 8 ? a.letter_table2[i] : 0.0;
    }
    // the credit tables travel with the launch and are read straight from the kernarg segment (see k_letters_cred8)
    static_assert(sizeof(ScanArgs) % alignof(PairCredTable) == 0, "ct follows a in the kernarg segment");
    (void)ct;
    typedef const __attribute__((address_space(4))) unsigned char *karg_ptr;
    const __attribute__((address_space(4))) uint32_t *ktab =
        (const __attribute__((address_space(4))) uint32_t *)((karg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(ScanArgs));
    for (int i = threadIdx.x; i < 2 * 8 * EDW; i += BLOCK) {
        const int s = i / (8 * EDW), e = i % (8 * EDW);
        ctab[s][e] = (e % EDW) < NJ ? ktab[s * 128 + (e / EDW) * 16 + (e % EDW)] : 0u;
    }
    const HitShard shard{a.hit_count, a.hit_shards, a.capacity};
    WaveHitQueue<float, PCS_QCAP, true> hq(hq_lds, a, shard, first);
    SurvivorQueue<decltype(hq)> sq(sv_pos[threadIdx.x >> 6], hq);
    hq.reset();
    park2(cbuf[0]);
    if (ntile > 1 && first + LET_TILE < n_pos) fetch2(first + LET_TILE);
    __syncthreads();

    const char *cb1 = (const char *)ctab[0], *cb2 = (const char *)ctab[1];
    // both exact scores of the survivor at stream position p (_pwm.c:34-68, matrix.py:25-43), then the whole predicate
    auto exact = [&](int64_t p) {
        const int64_t al = p & ~(int64_t)3;
        uint32_t raw[NRAW];
#pragma unroll
        for (int k = 0; k < NRAW; ++k) raw[k] = load_codes4(a.codes, al + 4 * k, n_pos);
        double sc = 0.0;
#pragma unroll
        for (int k = 0; k < NRAW - 1; ++k) {
            const uint32_t cw = __builtin_amdgcn_alignbyte(raw[k + 1], raw[k], (uint32_t)(p & 3));
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = 4 * k + b;
                if (j < TROWS) sc += tbl[0][j * 8 + ((cw >> (8 * b)) & 7u)];        // rows m .. 2 NJ - 1 are zeros
            }
        }
        const float f = (float)sc;
        if (!((double)f > a.thr_seq)) return;
#pragma unroll
        for (int k = 0; k < NRAW; ++k) raw[k] = load_codes4(a.codes2, al + 4 * k, n_pos);
        double st = 0.0;
#pragma unroll
        for (int k = 0; k < NRAW - 1; ++k) {
            const uint32_t cw = __builtin_amdgcn_alignbyte(raw[k + 1], raw[k], (uint32_t)(p & 3));
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = 4 * k + b;
                if (j < TROWS) st += tbl[1][j * 8 + ((cw >> (8 * b)) & 7u)];
            }
        }
        if (st > a.thr_struct && pair_sum_passes(f, st, a.thr_sum, a.sum_margin0)) hq.push((uint32_t)(p - first), f, st);
    };
    for (int tb = 0; tb < ntile; ++tb) {
        const int64_t tile0 = first + (int64_t)tb * LET_TILE;
        if (tile0 >= n_pos) break;                     // uniform; the previous tile flushed (it was the last)
        const uint8_t *cb = cbuf[tb & 1];
        const int off0 = threadIdx.x * W;
        // xs1 / xs2 byte k = (sequence / structure code at byte 4d + k) << PSH: an entry offset is one v_bfe_u32
        uint32_t xs1[NWD], xs2[NWD];
#pragma unroll
        for (int d = 0; d < NWD; ++d) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(cb + off0 + 4 * d);      // inside the halo
            xs1[d] = (w & 0x07070707u) << PSH;
            xs2[d] = ((w >> 3) & 0x07070707u) << PSH;
        }
        uint32_t pk[W + 1];
#pragma unroll
        for (int i = 0; i < W + 1; ++i) pk[i] = 0u;
        // q, g and k are constant expressions (static_for): every pk[] / dj[] index is a register name
        static_for<0, NPOS>([&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value;
            constexpr int KMAX = NJ - 1;
            constexpr int klo = q > W ? (q - W + 1) / 2 : 0, khi = q / 2 < KMAX ? q / 2 : KMAX;
            static_for<0, 2>([&](auto sc_) __attribute__((always_inline)) {
                constexpr int s = decltype(sc_)::value;
                const uint32_t xw = s == 0 ? xs1[q >> 2] : xs2[q >> 2];
                const char *cbytes = s == 0 ? cb1 : cb2;
                uint32_t off = (xw >> (8 * (q & 3))) & 0xFFu;
                if constexpr (ESTR == 80) off += off << 2;      // code * 16 * 5
                uint32_t dj[16] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                if constexpr (NJ <= 2) {
                    const u32x2 e = *reinterpret_cast<const u32x2 *>(cbytes + off);
                    dj[0] = e[0];
                    dj[1] = e[1];
                } else {
                    static_for<0, (NJ + 3) / 4>([&](auto gc) __attribute__((always_inline)) {
                        constexpr int g = decltype(gc)::value;
                        if constexpr (!(4 * g > khi || 4 * g + 3 < klo)) {
                            if constexpr (NJ - 4 * g >= 3) {
                                const u32x4 e = *reinterpret_cast<const u32x4 *>(cbytes + off + 16 * g);
                                dj[4 * g] = e[0];
                                dj[4 * g + 1] = e[1];
                                dj[4 * g + 2] = e[2];
                                dj[4 * g + 3] = e[3];
                            } else {                   // a last group of two row pairs (NJ = 6)
                                const u32x2 e = *reinterpret_cast<const u32x2 *>(cbytes + off + 16 * g);
                                dj[4 * g] = e[0];
                                dj[4 * g + 1] = e[1];
                            }
                        }
                    });
                }
                static_for<0, NJ>([&](auto kc) __attribute__((always_inline)) {
                    constexpr int k = decltype(kc)::value;
                    constexpr int u = q - 2 * k;       // rows 2k (lo: window u) and 2k + 1 (hi: window u - 1)
                    if constexpr (u >= 0 && u <= W) pk[u] += dj[k];
                });
            });
        });
        // the 16 sums two at a time, as k_letters_cred8: bit 15 of a sum (they stay below 2^16) is its flag
        uint32_t surv = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t x = __builtin_amdgcn_alignbit(pk[2 * k], pk[2 * k + 2], 16);
            const u16x2 r = __builtin_bit_cast(u16x2, pk[2 * k + 1]) + __builtin_bit_cast(u16x2, x);
            surv = (surv >> 1) | (__builtin_bit_cast(uint32_t, r) & 0x80008000u);
        }
        sq.hand_over(surv, (uint32_t)(tile0 - first), off0, [](int b) { return 2 * (b & 7) + (b < 16 ? 1 : 0); }, exact);

        const bool more = tb + 1 < ntile && tile0 + LET_TILE < n_pos;
        if (!more) sq.finish(exact);                   // last tile of the workgroup: the waiting survivors, then the final flush
        hq.tile_boundary(tb, more, [&]() { if (more) park2(cbuf[(tb + 1) & 1]); },
                         [&]() { if (tb + 2 < ntile && tile0 + 2 * (int64_t)LET_TILE < n_pos) fetch2(tile0 + 2 * (int64_t)LET_TILE); });
    }
}

// Host: the joint credit tables of one pair at thr_sum.  A hit has fl(fl(f + st) + mg) > thr_sum (pair_sum_maybe), so
// (double) f + st > thr_j := thr_sum - Mmax with Mmax >= mg + the rounding of the two additions for every window:
//     Mmax = 0.0010001 + 4.01 * 2^-24 F1 + 2^-48 (F1 + F2 + |thr_sum|),  F1 / F2 = sum_j max_c |cell| of either table (finite cells;
// |f| <= F1 (1 + 2^-23), |st| <= F2 (1 + m 2^-53)), every host operation rounded to the safe side.  build_credits then
// treats the 2 m rows of both tables as ONE motif at threshold thr_j: one quantum, one-sided rounding, the threshold in
// row 0, and its own delta = 2^-23 sum |cell| + 1e-9 covers the float32 cast of f and the fp64 summation errors of both sums.
// NaN cells count as -inf (such a window is NaN and never passes).  Switch-offs (mode 3): a +inf cell on either side,
// F1 beyond ROUND3_SAFE, a non-finite thr_j or quantum; widths above 32 are not this kernel's.  mode 2: dense.
void build_pair_credits(const double *L1, const double *L2, int m, double thr_sum, PairCred *pc)
{
    pc->mode = 3;
    pc->quantum = pc->slack = INFINITY;
    pc->thr_joint = thr_sum;
    std::fill(pc->cr, pc->cr + 64 * 8, (uint16_t)0);
    if (m < 1 || m > 32 || std::isnan(thr_sum)) return;
    std::vector<double> rows((size_t)2 * m * 8);
    double F[2] = {0.0, 0.0};
    int ncol[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
        const double *L = s ? L2 : L1;
        for (int j = 0; j < m; ++j) {
            double mx = 0.0;
            for (int c = 0; c < 8; ++c) {
                const double v = L[j * 8 + c];
                rows[((size_t)s * m + j) * 8 + c] = std::isnan(v) ? -INFINITY : v;
                if (std::isfinite(v)) mx = std::max(mx, std::fabs(v));
                if (!std::isnan(v)) ncol[s] = std::max(ncol[s], c + 1);
            }
            F[s] = next_up(F[s] + mx);
        }
    }
    if (!(F[0] <= ROUND3_SAFE)) return;
    double thr_j = thr_sum;
    if (std::isfinite(thr_sum)) {
        thr_j = next_down(thr_sum - pair_joint_margin(F[0], F[1], thr_sum));
    }
    if (std::isnan(thr_j)) return;
    pc->thr_joint = thr_j;
    if (thr_j == -INFINITY) return;                    // no joint threshold, nothing to fold in
    const double slack = build_credits(rows.data(), 2 * m, thr_j, pc->cr, 16, 8);
    if (!std::isfinite(slack)) {                       // +inf cell, non-finite quantum: the tables are not used
        std::fill(pc->cr, pc->cr + 64 * 8, (uint16_t)0);
        return;
    }
    pc->slack = slack;
    pc->quantum = slack / (2 * m);
    pc->mode = 1;
    // survivor rate for independent, uniformly drawn letters: the exact distribution of the 16-bit credit sum
    std::vector<double> dist(65536, 0.0), next(65536, 0.0);
    std::vector<int> support{0}, nsupport;
    dist[0] = 1.0;
    for (int r = 0; r < 2 * m; ++r) {
        const int nc = std::max(1, ncol[r >= m]);
        nsupport.clear();
        for (int v : support) {
            const double pv = dist[(size_t)v];
            for (int c = 0; c < nc; ++c) {
                const int w2 = std::min(65535, v + (int)pc->cr[r * 8 + c]);
                if (next[(size_t)w2] == 0.0) nsupport.push_back(w2);
                next[(size_t)w2] += pv / nc;
            }
            dist[(size_t)v] = 0.0;
        }
        dist.swap(next);
        support.swap(nsupport);
    }
    double survive = 0.0;
    for (int v : support)
        if (v >= 32768) survive += dist[(size_t)v];
    pc->survive = survive;
    if (survive > 1.0 / 32.0) pc->mode = 2;
}

// false: not applicable (width > 32, prefilter switched off, predicted survivor rate above 1/32) -> k_pair_sum_dense
bool launch_pair_cred_sum(const ScanArgs &a, const double *h_letters2, PairCred *cache, const Tuning &t, hipStream_t stream, hipError_t *err)
{
    if (!(a.hits && a.codes && a.codes2 && a.letter_table && a.letter_table2 && a.h_letters && h_letters2 && a.m <= 32 && t.credits &&
          std::isfinite(a.thr_sum)))
        return false;
    PairCredTable ct;
    int mode;
    {
        static std::mutex mu;                          // host threads that scan with one motif take turns; each launch carries its own table
        std::lock_guard<std::mutex> lock(mu);
        PairCred local, *pc = cache ? cache : &local;
        if (!(pc->mode != 0 && pc->thr_sum == a.thr_sum && pc->m == a.m && std::memcmp(pc->key2, h_letters2, sizeof(double) * 8 * a.m) == 0)) {
            build_pair_credits(a.h_letters, h_letters2, a.m, a.thr_sum, pc);
            pc->thr_sum = a.thr_sum;
            pc->m = a.m;
            std::memcpy(pc->key2, h_letters2, sizeof(double) * 8 * a.m);
        }
        mode = pc->mode;
        std::memset(&ct, 0, sizeof(ct));
        if (mode == 1)
            for (int s = 0; s < 2; ++s)
                for (int c = 0; c < 8; ++c)
                    for (int j = 0; j < a.m; ++j) ct.d[s][c][j >> 1] |= (uint32_t)pc->cr[(s * a.m + j) * 8 + c] << (16 * (j & 1));
    }
    if (mode != 1) return false;
    const int nj = (a.m + 1) / 2;
    constexpr int TILE = BLOCK * 16;
    ScanArgs b = a;
    const int64_t ntiles = (a.n_pos + TILE - 1) / TILE;
    const int64_t per = (int64_t)t.n_cu * 18;          // ~18 workgroups per CU in the grid (walk_tiles, pfmscan_kernels.hip)
    b.tiles_per_block = (int)std::min<int64_t>(32, std::max<int64_t>(1, (ntiles + per / 2) / per));
    if (t.tiles_per_block > 0) b.tiles_per_block = t.tiles_per_block;
    const unsigned g = (unsigned)((ntiles + b.tiles_per_block - 1) / b.tiles_per_block);
    if (nj <= 2) hipLaunchKernelGGL((k_pair_cred_sum<2>), dim3(g), dim3(BLOCK), 0, stream, b, ct);
    else if (nj <= 4) hipLaunchKernelGGL((k_pair_cred_sum<4>), dim3(g), dim3(BLOCK), 0, stream, b, ct);
    else if (nj <= 6) hipLaunchKernelGGL((k_pair_cred_sum<6>), dim3(g), dim3(BLOCK), 0, stream, b, ct);
    else if (nj <= 8) hipLaunchKernelGGL((k_pair_cred_sum<8>), dim3(g), dim3(BLOCK), 0, stream, b, ct);
    else if (nj <= 10) hipLaunchKernelGGL((k_pair_cred_sum<10>), dim3(g), dim3(BLOCK), 0, stream, b, ct);
    else if (nj <= 12) hipLaunchKernelGGL((k_pair_cred_sum<12>), dim3(g), dim3(BLOCK), 0, stream, b, ct);
    else hipLaunchKernelGGL((k_pair_cred_sum<16>), dim3(g), dim3(BLOCK), 0, stream, b, ct);
    *err = hipGetLastError();
    return true;
}

// a.codes / a.letter_table: the sequence side, a.codes2 / a.letter_table2: the structure side; hit fields as fill_hits left them
hipError_t launch_pair_sum_dense(const ScanArgs &a, hipStream_t stream)
{
    if (!a.codes || !a.codes2 || !a.letter_table || !a.letter_table2 || a.m < 1 || a.m > PFMSCAN_MAX_WIDTH) return hipErrorInvalidValue;
    if (a.n_pos <= 0) return hipSuccess;
    const int64_t grid = (a.n_pos + PSD_TILE - 1) / PSD_TILE;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pair_sum_dense, dim3((unsigned)grid), dim3(BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pfmscan
