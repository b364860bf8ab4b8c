// pfmscan_fp.hpp -- the host side the two posterior site maps share (pfmscan_footprint.hip over letter codes,
// pfmscan_footprint_profile.hip over averaged-structure profiles): what a call leaves, the check of the event buffers, and the
// way home of a _staged form's events (room on the device, then the count, the capacity verdict and the sort by key).
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "pfmscan_ctx.hpp"
#include "pfmscan_occ.hpp"

namespace pfmscan {

// what a call leaves: the maps (either may be null), or with events the positions whose cover passes thr
struct FpOut {
    double *start, *cover;
    bool events;
    double thr;
    int64_t capacity;
    int64_t *ev_key;
    double *ev_cover, *ev_start;
    unsigned long long *ev_count;
};

inline int fp_check_events(pfmscan_ctx *ctx, const char *who, double thr, int64_t capacity, const void *count, const void *key, const void *cover,
                           const void *start)
{
    if (std::isnan(thr)) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": NaN threshold");
    if (capacity < 0 || !count || (capacity > 0 && (!key || !cover || !start))) return fail(ctx, PFMSCAN_E_BADARG, std::string(who) + ": bad event buffers");
    return PFMSCAN_OK;
}

// Room for the events of a _staged form (ctx->fp_ev: keys, covers, starts of max(capacity, 1) events), its occupancy and window
// counts (ctx->fp_out; null where the caller takes none) and the counter (ctx->count, zeroed on ctx->stream) -> the FpOut of the call
inline int fp_events_room(pfmscan_ctx *ctx, double thr, int64_t capacity, size_t pairs, size_t n_rec, bool want_occ, bool want_windows, FpOut &o,
                          double *&d_occ, int64_t *&d_win)
{
    int rc;
    const size_t cap = (size_t)std::max<int64_t>(capacity, 1);
    if ((rc = ensure(ctx, ctx->fp_ev, cap * 24))) return rc;
    if ((rc = ensure(ctx, ctx->fp_out, (pairs + n_rec) * 8))) return rc;
    if ((rc = ensure(ctx, ctx->count, HIT_COUNTER_STRIDE * 8))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->count.p, 0, 8, ctx->stream));
    int64_t *d_key = (int64_t *)ctx->fp_ev.p;
    double *d_cov = (double *)ctx->fp_ev.p + cap, *d_sta = d_cov + cap;
    d_occ = want_occ ? (double *)ctx->fp_out.p : nullptr;
    d_win = want_windows ? (int64_t *)ctx->fp_out.p + pairs : nullptr;
    o = FpOut{nullptr, nullptr, true, thr, capacity, d_key, d_cov, d_sta, (unsigned long long *)ctx->count.p};
    return PFMSCAN_OK;
}

// The tail of a _staged events form, after its pass was launched on ctx->stream: the count comes home (*n_events; beyond the
// capacity: PFMSCAN_E_CAPACITY, nothing written), then the events, the occupancy and the window counts (null: not asked for);
// the keys are distinct and are sorted on the host, as the mutagenesis events are
inline int fp_events_home(pfmscan_ctx *ctx, const char *who, const FpOut &o, int64_t *ev_key, double *ev_cover, double *ev_start, int64_t *n_events,
                          const OccHome &occ, const OccHome &windows)
{
    uint64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, o.ev_count, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_events = (int64_t)total;
    if ((int64_t)total > o.capacity)
        return fail(ctx, PFMSCAN_E_CAPACITY, std::string(who) + ": " + std::to_string(total) + " events, capacity " + std::to_string(o.capacity));
    std::vector<int64_t> key(total);
    std::vector<double> cv(total), sw(total);
    if (total) {
        HIP_TRY(ctx, hipMemcpyAsync(key.data(), o.ev_key, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(cv.data(), o.ev_cover, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(sw.data(), o.ev_start, total * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (int rc = occ_copy_home(ctx, {occ, windows})) return rc;
    std::vector<int64_t> order(total);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key[x] < key[y]; });
    for (uint64_t i = 0; i < total; ++i) {
        ev_key[i] = key[order[i]];
        ev_cover[i] = cv[order[i]];
        ev_start[i] = sw[order[i]];
    }
    return PFMSCAN_OK;
}

}  // namespace pfmscan
