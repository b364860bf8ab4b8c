// pfmscan_hits.hpp -- the host side of the sharded hit buffers (bodies in pfmscan_hits.hip): every thresholded entry
// point that returns hits sizes a sink, zeroes its counters, launches, reads the counters back, decides
// PFMSCAN_E_CAPACITY and sorts the hits home through the helpers below.  Not installed.
//
// A sink is `shards` regions of `shard_cap` slots with one counter per region, HIT_COUNTER_STRIDE words apart: workgroup b
// appends to shard b & (shards - 1).  A shard that overflowed while the total still fits has dropped hits, so the
// verdict looks at the fullest shard as well as at the sum.
#pragma once
#include <cmath>
#include <functional>

#include "pfmscan_ctx.hpp"

namespace pfmscan {

struct HitSink {                 // where hits go
    int64_t *pos;
    int32_t *motif;              // null: single-motif scan
    float *seq;
    double *st;
    unsigned long long *count;   // shards counters, HIT_COUNTER_STRIDE words apart (zeroed by acquire_sink, or by the caller of a _dev form)
    int shards;
    int64_t shard_cap;
};

// the ctx buffers a sink lives in (null: the scan has no such column)
struct SinkBufs {
    DevBuf *pos, *motif, *seq, *st, *count;
    size_t count_bytes;          // of `count` when it holds more than the counters (0: shards counters)
};
inline SinkBufs hit_bufs(pfmscan_ctx *ctx) { return {&ctx->hit_pos, nullptr, &ctx->hit_seq, &ctx->hit_struct, &ctx->count, 0}; }
inline SinkBufs cand_bufs(pfmscan_ctx *ctx) { return {&ctx->cand_pos, nullptr, &ctx->cand_seq, nullptr, &ctx->cand_count, 0}; }

// lib_count: LIB_SHARDS counters and two spare lines, then starts[LIB_SHARDS + 1] of k_lib_prefix / k_lib_pack
constexpr size_t LIB_STARTS_OFFSET = (size_t)(LIB_SHARDS + 2) * HIT_COUNTER_STRIDE * 8;
constexpr size_t LIB_COUNT_BYTES = LIB_STARTS_OFFSET + (LIB_SHARDS + 1) * 8;
inline SinkBufs lib_bufs(pfmscan_ctx *ctx) { return {&ctx->lib_pos, &ctx->lib_motif, &ctx->lib_seq, &ctx->lib_struct, &ctx->lib_count, LIB_COUNT_BYTES}; }
inline int64_t *lib_starts(const HitSink &k) { return reinterpret_cast<int64_t *>(reinterpret_cast<unsigned char *>(k.count) + LIB_STARTS_OFFSET); }

// Slots per shard.  Single motif: shard s = workgroup & 31 gets every 32nd tile, so the shards fill evenly and each has
// room for twice its share (small streams have few workgroups, i.e. few shards in use: there every shard can take everything).
inline int64_t hit_shard_cap(int64_t capacity)
{
    return std::max<int64_t>(std::min<int64_t>(capacity, capacity / HIT_SHARDS * 2 + 4096), 1);
}
// Library: shard s = workgroup & 255 gets every 256th work unit (`work_unit` positions per workgroup visit): the shards in
// use fill evenly, each has room for twice its share (short streams use few shards, small capacities let every shard take
// everything).
inline int64_t lib_shard_cap(int64_t capacity, int64_t n_pos, int64_t work_unit)
{
    const int64_t active = std::max<int64_t>(1, std::min<int64_t>(LIB_SHARDS, (n_pos + work_unit - 1) / work_unit));
    return std::max<int64_t>(std::min<int64_t>(capacity, capacity / active * 2 + 1024), 1);
}
// Candidates of the letters pass of the candidate-then-verify combined scan: room for `cand_cap` of them in all.
inline int64_t cand_shard_cap(int64_t cand_cap) { return std::min<int64_t>(cand_cap, cand_cap / HIT_SHARDS * 2 + 4096); }
// Candidates of the two-FASTA scan: 1/32 of the windows, twice a shard's share.
inline int64_t pair_cand_shard_cap(int64_t n_pos) { return std::max<int64_t>(n_pos / 32 / HIT_SHARDS * 2 + 4096, 1); }

// grows `b` to `shards` regions of `shard_cap` slots, zeroes the counters on `st` -> sink
int acquire_sink(pfmscan_ctx *ctx, const SinkBufs &b, int shards, int64_t shard_cap, hipStream_t st, HitSink &sink);
// the hit fields of `a` from a sink; has_seq / has_struct: which score columns the launch writes
// thr_sum: the joint threshold on the printed LogOdds.SeqStruct (pfmscan_hits_sum_*; needs both score columns); -inf = none
void fill_hits(ScanArgs &a, const HitSink &k, bool has_seq, bool has_struct, double thr_seq, double thr_struct, double thr_sum = -INFINITY);
// the pfmscan_hits_sum_* argument check: both parts, no NaN
int check_sum(pfmscan_ctx *ctx, const pfmscan_motif *mo, double thr_sum);
// counters -> host: their sum and the fullest shard.  Synchronises `st`.
int read_hit_counts(pfmscan_ctx *ctx, const unsigned long long *d_count, int shards, hipStream_t st, uint64_t &total, uint64_t &worst);
// A sink filled on ctx->stream -> the caller's host arrays, sorted by position (by (position, motif) when the sink has a
// motif column: n_motifs sizes its key bits): capacity verdict, device sort (pfmscan_sort.hip), contiguous copies, NaN in
// the score column the scan does not have.  Synchronises ctx->stream.  Hit positions lie in [0, n_pos).
int finish_sorted_hits(pfmscan_ctx *ctx, const HitSink &sink, bool has_seq, bool has_struct, int n_motifs, int64_t n_pos, int64_t capacity,
                       int64_t *hit_pos, int32_t *hit_motif, float *hit_seq, double *hit_struct, int64_t *n_hits);

// pfmscan_pipeline.hip: a HOST-resident stream through two alternating device buffers (ctx->pipe_codes / pipe_profile; null
// codes / row_bytes 0: no such side), the upload of chunk k + 1 on the copy stream beside the scan of chunk k.  A chunk is
// chunk_positions long plus an overhang of m - 1; scan(b, a0, len) launches the scan of buffer b, which holds the `len`
// positions from a0 on, on ctx->stream.  Synchronises the copy stream.
int pipeline_chunks(pfmscan_ctx *ctx, const uint8_t *codes, const void *profile, size_t row_bytes, int64_t n_pos, int64_t chunk_positions,
                    int m, const std::function<int(int b, int64_t a0, int64_t len)> &scan);

}  // namespace pfmscan
