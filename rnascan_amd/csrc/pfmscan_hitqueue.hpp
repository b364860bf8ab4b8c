// pfmscan_hitqueue.hpp -- the DEVICE side of the sharded hit protocol: which shard a workgroup appends to and how slots are
// reserved (HitShard), the wave-private LDS hit queue of k_letters_pre and k_letters_cred8 (WaveHitQueue) and the survivor
// queue in front of it (SurvivorQueue).  k_letters_cred and phase B of k_library / k_library8 still spell the same protocol
// out: moved onto these helpers hipcc compiles them to different code, and they keep what was measured.  The host side of the same layout -- sizing, counter read-back, the capacity verdict, the sorted copy
// home -- is pfmscan_hits.hpp.  Not installed.
#pragma once
#include "pfmscan_internal.hpp"

namespace pfmscan {

// The shard of the hit buffers this workgroup appends to: workgroup b -> shard b & (hit_shards - 1), slots
// [shard * capacity, (shard + 1) * capacity), counter HIT_COUNTER_STRIDE words after the previous shard's.  `capacity`
// is PER SHARD, here and in every kernel's arguments (a HitSink's shard_cap, pfmscan_hits.hpp): a slot at or beyond it
// is counted, never stored, and the host reports PFMSCAN_E_CAPACITY from the counters.
struct HitShard {
    unsigned long long *hit_count;
    int hit_shards;
    int64_t capacity;
    // derived where they are used (wave-uniform scalar arithmetic on kernel arguments): a workgroup that reports no hit
    // never computes them.  (The counter offset is an int product, at most 64 shards x 16 words: emit_hits_block has always
    // computed it so, and the kernels that use it compile to the instructions they had.)
    __device__ __forceinline__ unsigned index() const { return blockIdx.x & (hit_shards - 1); }
    __device__ __forceinline__ unsigned long long *counter() const { return hit_count + (int)index() * HIT_COUNTER_STRIDE; }
    __device__ __forceinline__ unsigned long long off() const { return (unsigned long long)index() * (unsigned long long)capacity; }   // the shard's first slot
    // n slots -> the first one; ONE thread (a returning atomic: sharded, because one word saturates at ~88 atomics/us)
    __device__ __forceinline__ unsigned long long reserve(unsigned long long n) const { return atomicAdd(counter(), n); }
    // lane 0 reserves n slots, every lane of the wave learns the base (wave-uniform: two scalar reads)
    __device__ __forceinline__ unsigned long long reserve_wave(int n) const
    {
        unsigned long long base = 0;
        if ((threadIdx.x & 63) == 0) base = reserve((unsigned long long)n);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base), hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
        return ((unsigned long long)hi << 32) | lo;
    }
    __device__ __forceinline__ bool in_range(unsigned long long slot) const { return (int64_t)slot < capacity; }
};

constexpr int HQ_WAVES = 4;                            // the tile-walking kernels run 256-thread workgroups
constexpr int WQ_CAP = 256;                            // hits a wave can park: k_letters_pre / _cred (8 bytes each; 16 with the second score: half as many)
constexpr int Q8_CAP = 128;                            // k_letters_cred8 (12 bytes each)
constexpr int SV_CAP = 128;                            // survivors a wave can park: fewer than 64 waiting + the 64 of one pass

// LDS of a workgroup's hit queues (one __shared__ object per kernel; no padding: 8-byte members first, a multiple of 16
// bytes in all).  Positions are relative to the workgroup's first tile (4 bytes: 22.7 instead of 26.8 KB of LDS in
// k_letters_pre).
template <int CAP, bool SECOND> struct HitQueueSecond { double st[HQ_WAVES][CAP]; };
template <int CAP> struct HitQueueSecond<CAP, false> {};
template <typename SCORE_T, int CAP, bool SECOND> struct HitQueueLds : HitQueueSecond<CAP, SECOND> {
    SCORE_T sc[HQ_WAVES][CAP];
    uint32_t pos[HQ_WAVES][CAP];
    int n[HQ_WAVES], snap[2][HQ_WAVES];
};

// Hits are rare and found in divergent code, so they are not scanned into place: a hit lane takes a slot of its WAVE's
// queue with an LDS atomic.  The queue lives across the tiles a workgroup walks; at a tile boundary the four queues are
// flushed with ONE returning global atomic once one of them is half full, and at the end (tile_boundary); a wave whose queue
// cannot take the hits the next step may bring flushes alone (ensure_room: dense stretches only).  Hits land in no
// particular order; the host sorts.  A hit is (position, score[, second score]); its columns in the hit buffers are
// hit_seq = (float)score and hit_struct = the second score, or (double)score where there is none.
// LDS operations of one wave execute in order; the fences keep the COMPILER from moving LDS accesses of other lanes'
// data across the points where lanes change roles.
template <typename SCORE_T, int CAP, bool SECOND> struct WaveHitQueue {
    static_assert(sizeof(HitQueueLds<SCORE_T, CAP, SECOND>) % 16 == 0, "the queues pad the workgroup's LDS");
    HitQueueLds<SCORE_T, CAP, SECOND> &q;
    const ScanArgs &a;
    const HitShard &shard;
    const int64_t first;                               // the workgroup's first stream position
    const int lane, wave;
    int ub = 0;                                        // wave-uniform upper bound of q.n[wave]

    __device__ __forceinline__ WaveHitQueue(HitQueueLds<SCORE_T, CAP, SECOND> &lds, const ScanArgs &args, const HitShard &sh, int64_t first_pos)
        : q(lds), a(args), shard(sh), first(first_pos), lane(threadIdx.x & 63), wave(threadIdx.x >> 6) {}

    // before the kernel's first barrier
    __device__ __forceinline__ void reset()
    {
        if (threadIdx.x < HQ_WAVES) q.n[threadIdx.x] = 0;
    }
    __device__ __forceinline__ void push(uint32_t rel_pos, SCORE_T sc, double st = 0.0)
    {
        const int slot = atomicAdd(&q.n[wave], 1);     // LDS
        q.pos[wave][slot] = rel_pos;
        q.sc[wave][slot] = sc;
        if constexpr (SECOND) q.st[wave][slot] = st;
    }
    // this wave's queue -> global at base; all 64 lanes
    __device__ __forceinline__ void drain(unsigned long long base, int n)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < n; i += 64) {
            const unsigned long long slot = base + i;
            const int64_t pos = first + (int64_t)q.pos[wave][i];
            const SCORE_T sc = q.sc[wave][i];
            double st = (double)sc;
            if constexpr (SECOND) st = q.st[wave][i];
            if (shard.in_range(slot)) {
                a.hit_pos[shard.off() + slot] = pos + a.pos_offset;
                if (a.hit_seq) a.hit_seq[shard.off() + slot] = (float)sc;
                if (a.hit_struct) a.hit_struct[shard.off() + slot] = st;
            }
        }
        if (lane == 0) q.n[wave] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void wave_flush()
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int n = __builtin_amdgcn_readfirstlane(q.n[wave]);
        if (n == 0) return;
        drain(shard.reserve_wave(n), n);
    }
    // room for cnt more hits (wave-uniform cnt), which the caller may push next
    __device__ __forceinline__ void ensure_room(int cnt)
    {
        if (ub + cnt > CAP) {
            wave_flush();
            ub = 0;
        }
        ub += cnt;
    }
    // End of tile tb, all 256 threads: publish the next tile's codes (park) and this wave's queue length with ONE barrier,
    // start the loads of the tile after (fetch), flush when a queue is half full or no tile follows (`more` false).
    template <typename ParkF, typename FetchF> __device__ __forceinline__ void tile_boundary(int tb, bool more, ParkF park, FetchF fetch)
    {
        // the base of the workgroup-wide reservation, thread 0 -> everybody.  Not a member of HitQueueLds: hipcc aligns
        // every LDS object of this size to 16 bytes, the queues are a multiple of 16 bytes without this word, and with it
        // each kernel's LDS grows by 8 bytes of padding (measured: 18136 -> 18144 in k_letters_pre<5>)
        __shared__ unsigned long long s_base;
        park();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) q.snap[tb & 1][wave] = q.n[wave];
        __syncthreads();
        fetch();
        int nq[HQ_WAVES], total = 0, most = 0, before = 0;
#pragma unroll
        for (int k = 0; k < HQ_WAVES; ++k) {
            nq[k] = q.snap[tb & 1][k];
            if (k < wave) before += nq[k];
            total += nq[k];
            most = most > nq[k] ? most : nq[k];
        }
        ub = nq[wave];
        if (most >= CAP / 2 || (!more && total > 0)) {             // uniform: every thread read the same snapshot
            if (threadIdx.x == 0) s_base = shard.reserve((unsigned long long)total);
            __syncthreads();
            drain(s_base + (unsigned long long)before, nq[wave]);
            ub = 0;
        }
    }
};

// The survivors of an integer prefilter (k_letters_cred8; k_letters_cred holds its own copy, see there) waiting for their exact score: positions only, in a
// wave-private LDS queue that lives across tiles; 64 at a time they are scored one per lane.  score(p) computes the exact
// score of the window at stream position p and pushes it to the hit queue when it is a hit.
template <typename QUEUE> struct SurvivorQueue {
    uint32_t *const sv;                                // this wave's SV_CAP entries, relative to the workgroup's first tile
    QUEUE &hq;
    int n = 0;                                         // wave-uniform length (< 64 between tiles)

    __device__ __forceinline__ SurvivorQueue(uint32_t *wave_lds, QUEUE &hits) : sv(wave_lds), hq(hits) {}

    // exact score of survivors [at, at + cnt), one per lane
    template <typename ScoreF> __device__ __forceinline__ void exact_batch(int at, int cnt, ScoreF score)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        hq.ensure_room(cnt);                           // a hit per lane
        if (hq.lane < cnt) score(hq.first + (int64_t)sv[at + hq.lane]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // `surv`: the lane's flag bits of one tile, window_of(bit) the window (0 .. 15 of the lane's 16 at off0) a bit stands for.
    // ONE rolled loop, every pass each lane that still has a survivor hands over its lowest one: at -m 6 a sixth of the
    // (wave, window slot) pairs holds a survivor, and the unrolled pass per slot (test, ballot, branch, push) cost 3.3 of
    // k_letters_cred's 12.3 VALU instructions per window, this form 1.1; unrolled, the exact score was also inlined 17
    // times: 25 k instructions and 57 spilled SGPRs in the widest k_letters_cred8.
    template <typename WinF, typename ScoreF>
    __device__ __forceinline__ void hand_over(uint32_t surv, uint32_t tile_rel, int off0, WinF window_of, ScoreF score)
    {
        while (__builtin_amdgcn_ballot_w64(surv != 0)) {
            const bool s = surv != 0;
            const unsigned long long sb = __builtin_amdgcn_ballot_w64(s);
            if (s) {
                const int b = __builtin_ctz(surv);
                surv &= surv - 1;
                sv[n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(sb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sb, 0u))] = tile_rel + (uint32_t)(off0 + window_of(b));
            }
            n += __popcll(sb);
            if (n >= 64) {                             // the top 64 get their exact score, the rest stays
                exact_batch(n - 64, 64, score);
                n -= 64;
            }
        }
    }
    // the workgroup's last tile: the waiting survivors
    template <typename ScoreF> __device__ __forceinline__ void finish(ScoreF score)
    {
        if (n > 0) {
            exact_batch(0, n, score);
            n = 0;
        }
    }
};

}  // namespace pfmscan
