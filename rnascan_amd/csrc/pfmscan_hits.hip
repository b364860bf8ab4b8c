// pfmscan_hits.hip -- the host side of the sharded hit buffers (pfmscan_hits.hpp): sizing and zeroing a sink, the counter
// read-back, the capacity verdict and the sorted copy home.  Host code only; the kernels it launches are pfmscan_sort.hip's.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pfmscan_hits.hpp"
#include "pfmscan_exact.hpp"

namespace pfmscan {

int acquire_sink(pfmscan_ctx *ctx, const SinkBufs &b, int shards, int64_t shard_cap, hipStream_t st, HitSink &sink)
{
    int rc;
    const size_t slots = (size_t)shard_cap * shards;
    const size_t counter_bytes = (size_t)shards * HIT_COUNTER_STRIDE * 8;
    if ((rc = ensure(ctx, *b.pos, slots * 8))) return rc;
    if (b.motif && (rc = ensure(ctx, *b.motif, slots * 4))) return rc;
    if (b.seq && (rc = ensure(ctx, *b.seq, slots * 4))) return rc;
    if (b.st && (rc = ensure(ctx, *b.st, slots * 8))) return rc;
    if ((rc = ensure(ctx, *b.count, std::max(counter_bytes, b.count_bytes)))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(b.count->p, 0, counter_bytes, st));
    sink.pos = (int64_t *)b.pos->p;
    sink.motif = b.motif ? (int32_t *)b.motif->p : nullptr;
    sink.seq = b.seq ? (float *)b.seq->p : nullptr;
    sink.st = b.st ? (double *)b.st->p : nullptr;
    sink.count = (unsigned long long *)b.count->p;
    sink.shards = shards;
    sink.shard_cap = shard_cap;
    return PFMSCAN_OK;
}

int check_sum(pfmscan_ctx *ctx, const pfmscan_motif *mo, double thr_sum)
{
    if (!ctx || !mo) return fail(ctx, PFMSCAN_E_BADARG, "NULL ctx or motif");
    if (!mo->d_letters || !mo->d_struct)
        return fail(ctx, PFMSCAN_E_BADARG, "a threshold on LogOdds.SeqStruct needs a motif with a letter table AND a structure PSSM");
    if (std::isnan(thr_sum)) return fail(ctx, PFMSCAN_E_BADARG, "NaN threshold");
    return PFMSCAN_OK;
}

void fill_hits(ScanArgs &a, const HitSink &k, bool has_seq, bool has_struct, double thr_seq, double thr_struct, double thr_sum)
{
    a.hits = 1;
    a.thr_seq = thr_seq;
    a.thr_struct = thr_struct;
    a.thr_sum = (has_seq && has_struct) ? thr_sum : -INFINITY;
    a.sum_band = sum_band(a.struct_band, a.thr_sum);
    a.sum_margin0 = sum_margin0(a.sum_band);
    a.capacity = k.shard_cap;
    a.hit_pos = k.pos;
    a.hit_seq = has_seq ? k.seq : nullptr;
    a.hit_struct = has_struct ? k.st : nullptr;
    a.hit_count = k.count;
    a.hit_shards = k.shards;
}

int read_hit_counts(pfmscan_ctx *ctx, const unsigned long long *d_count, int shards, hipStream_t st, uint64_t &total, uint64_t &worst)
{
    std::vector<unsigned long long> counters((size_t)shards * HIT_COUNTER_STRIDE);
    HIP_TRY(ctx, hipMemcpyAsync(counters.data(), d_count, counters.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    total = worst = 0;
    for (int s = 0; s < shards; ++s) {
        total += counters[(size_t)s * HIT_COUNTER_STRIDE];
        worst = std::max<uint64_t>(worst, counters[(size_t)s * HIT_COUNTER_STRIDE]);
    }
    return PFMSCAN_OK;
}

int finish_sorted_hits(pfmscan_ctx *ctx, const HitSink &sink, bool has_seq, bool has_struct, int n_motifs, int64_t n_pos, int64_t capacity,
                       int64_t *hit_pos, int32_t *hit_motif, float *hit_seq, double *hit_struct, int64_t *n_hits)
{
    int rc;
    hipStream_t st = ctx->stream;
    uint64_t total = 0, worst = 0;
    if ((rc = read_hit_counts(ctx, sink.count, sink.shards, st, total, worst))) return rc;
    *n_hits = (int64_t)total;
    if ((int64_t)total > capacity || (int64_t)worst > sink.shard_cap) {
        // ask for enough that every shard fits next time
        *n_hits = (int64_t)std::max<uint64_t>(total, worst * sink.shards);
        return fail(ctx, PFMSCAN_E_CAPACITY, "hit buffer too small: " + std::to_string(total) + " hits, capacity " + std::to_string(capacity));
    }
    if (total == 0) return PFMSCAN_OK;
    // shards -> one run in position order (libraries: (position, motif) order) on the device; contiguous copies come back
    int key_bits = 1, motif_bits = 0;
    if (sink.motif) {
        motif_bits = 1;
        while (key_bits < 62 && ((int64_t)1 << key_bits) < n_pos) ++key_bits;
        while (motif_bits < 16 && (1 << motif_bits) < n_motifs) ++motif_bits;
        if (key_bits + motif_bits > 63) return fail(ctx, PFMSCAN_E_BADARG, "stream too long for the (position, motif) sort key");
    } else {
        while (key_bits < 63 && ((int64_t)1 << key_bits) < n_pos) ++key_bits;
    }
    size_t temp_bytes = 0;
    HIP_TRY(ctx, sort_temp_bytes((int64_t)total, key_bits + motif_bits, &temp_bytes));
    if ((rc = ensure(ctx, ctx->sort_keys_in, total * 8))) return rc;
    if ((rc = ensure(ctx, ctx->sort_keys_out, total * 8))) return rc;
    if ((rc = ensure(ctx, ctx->sort_vals_in, total * 8))) return rc;
    if ((rc = ensure(ctx, ctx->sort_vals_out, total * 8))) return rc;
    if ((rc = ensure(ctx, ctx->sort_temp, std::max<size_t>(temp_bytes, 256)))) return rc;
    if ((rc = ensure(ctx, ctx->sort_seq, total * 4))) return rc;
    if ((rc = ensure(ctx, ctx->sort_struct, total * 8))) return rc;
    if (sink.motif && (rc = ensure(ctx, ctx->sort_motif, total * 4))) return rc;
    GatherArgs g;
    g.hit_pos = sink.pos;
    g.hit_seq = has_seq ? sink.seq : nullptr;
    g.hit_struct = has_struct ? sink.st : nullptr;
    g.counts = sink.count;
    g.shards = sink.shards;
    g.shard_cap = sink.shard_cap;
    g.total = (int64_t)total;
    g.key_bits = key_bits;
    g.keys_in = (int64_t *)ctx->sort_keys_in.p;
    g.keys_out = (int64_t *)ctx->sort_keys_out.p;
    g.vals_in = (int64_t *)ctx->sort_vals_in.p;
    g.vals_out = (int64_t *)ctx->sort_vals_out.p;
    g.temp = ctx->sort_temp.p;
    g.temp_bytes = ctx->sort_temp.cap;
    g.seq_out = (float *)ctx->sort_seq.p;
    g.struct_out = (double *)ctx->sort_struct.p;
    if (sink.motif) {
        g.hit_motif = sink.motif;
        g.motif_out = (int32_t *)ctx->sort_motif.p;
        g.motif_bits = motif_bits;
    }
    {
        hipError_t e = launch_gather_sorted(g, st);
        if (e != hipSuccess) return fail_hip(ctx, e, sink.motif ? "gather + sort of the library hits" : "gather + sort of the hits");
    }
    HIP_TRY(ctx, hipMemcpyAsync(hit_pos, g.keys_out, total * 8, hipMemcpyDeviceToHost, st));
    if (sink.motif) HIP_TRY(ctx, hipMemcpyAsync(hit_motif, g.motif_out, total * 4, hipMemcpyDeviceToHost, st));
    if (hit_seq && has_seq) HIP_TRY(ctx, hipMemcpyAsync(hit_seq, g.seq_out, total * 4, hipMemcpyDeviceToHost, st));
    if (hit_struct && has_struct) HIP_TRY(ctx, hipMemcpyAsync(hit_struct, g.struct_out, total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (hit_seq && !has_seq) std::fill(hit_seq, hit_seq + total, NAN);
    if (hit_struct && !has_struct) std::fill(hit_struct, hit_struct + total, (double)NAN);
    return PFMSCAN_OK;
}

}  // namespace pfmscan
