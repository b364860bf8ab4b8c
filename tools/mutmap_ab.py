"""Measurements of the in-silico mutagenesis entry points at C2 size (100k records x 3 kb, codes made on the
device), HIP-event times on one stream, the routes taking turns inside every repetition IN THE SAME JOB:

  route A   `pfmscan_mutmap_dev` with `where`: every position x 4 letters in one pass over the codes;
  route B   the 3 m + 1 `pfmscan_scan_dev` all-scores passes the composite route needs (3 m mutated streams whose mutated
            positions lie m apart, and the unmutated one) -- the device time of the passes ALONE, on the same codes: making
            the mutated streams and the max over the covering windows are left out, so this is a lower bound of that route;
  events    `pfmscan_mutmap_events_dev` at -m 6 (the counter's memset included);
  variants  `pfmscan_variants_dev`, 10^6 variants x 256 motifs.

for m = 8 and m = 12, each 5 times after warm-up: medians and the spread (min, max) are reported, and the map's ref column is
compared with the max over the covering windows of the plain scan at the size timed.  Run it under `rocprofv3 --kernel-trace
--stats` for kernel times, and under `--pmc` in a run of its own for counters.

    python tools/mutmap_ab.py [--records 100000] [--length 3000] [--widths 8,12] [--iters 5] [--warmup 2]
                              [--variants 1000000] [--motifs 256] [--thr 6] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pssm_table(rng, m):
    """a log-odds table as `rnascan -u -C 0.01` builds it from a random PFM: log2((p + c) / (1 + 4 c) / 0.25)"""
    p = rng.dirichlet(np.full(4, 0.4), size=m)
    T = np.full((m, 8), np.nan)
    T[:, :4] = np.log2((p + 0.01) / 1.04 / 0.25)
    return T


def timed_alternating(calls, iters, warmup):
    """{name: [ms]}: the calls take turns inside every repetition, each between two events of the stream it runs on"""
    import torch
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name in calls)
    for _ in range(iters):
        for name, call in calls.items():
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "ms": ms}


def ref_column_check(torch, codes, best, scores, m, n_check):
    """best[p][codes[p]] == max over j < m of scores[p - j] (NaN windows skipped) on the first n_check positions"""
    sc = torch.nan_to_num(scores[:n_check], nan=-float("inf"))
    top = torch.full_like(sc, -float("inf"))
    for j in range(m):
        top[j:] = torch.maximum(top[j:], sc[:n_check - j])
    c = codes[:n_check].long()
    ok = c < 4
    got = best[:n_check].gather(1, c.clamp(max=3)[:, None])[:, 0]
    want = torch.where(torch.isinf(top), torch.full_like(top, float("nan")), top)
    same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
    return bool(same[ok].all()) and bool(torch.isnan(best[:n_check][~ok]).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--widths", default="8,12")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", type=int, default=1000000)
    ap.add_argument("--motifs", type=int, default=256)
    ap.add_argument("--thr", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib
    n_rec, L = args.records, args.length
    n_pos = n_rec * (L + 1)
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    # the library's launches and the events share ONE stream of torch's.  Not the default stream: its handle is NULL, which
    # the library reads as "the ctx's own stream", and the events would bracket the enqueue, not the work
    side = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream != 0
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    codes = torch.randint(0, 4, (n_pos,), dtype=torch.uint8, device=dev, generator=g)
    codes.view(n_rec, L + 1)[:, L] = 7
    best = torch.empty((n_pos, 4), dtype=torch.float32, device=dev)
    where = torch.empty((n_pos, 4), dtype=torch.int8, device=dev)
    scores = torch.empty(n_pos, dtype=torch.float32, device=dev)
    cap = n_pos // 4
    ev_key = torch.empty(cap, dtype=torch.int64, device=dev)
    ev_ref = torch.empty(cap, dtype=torch.float32, device=dev)
    ev_alt = torch.empty(cap, dtype=torch.float32, device=dev)
    ev_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "thr": args.thr,
           "device": ctx.device_info()}
    for m in [int(x) for x in args.widths.split(",")]:
        T = pssm_table(rng, m)
        mo = ctx.motif(T)

        def route_a():
            ctx.mutmap_dev(mo, codes.data_ptr(), n_pos, best.data_ptr(), where.data_ptr(), stream)

        def route_b():
            for _ in range(3 * m + 1):
                ctx.scan_dev(mo, codes.data_ptr(), None, _lib.PROFILE_NONE, n_pos, scores.data_ptr(), None, stream)

        def events():
            ev_cnt.zero_()
            ctx.mutmap_events_dev(mo, codes.data_ptr(), n_pos, args.thr, cap, ev_key.data_ptr(), ev_ref.data_ptr(), ev_alt.data_ptr(),
                                  ev_cnt.data_ptr(), stream)

        times = timed_alternating({"A_mutmap_dev_with_where": route_a, "B_scan_dev_passes_alone": route_b, "mutmap_events_dev": events},
                                  args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry["B_passes"] = 3 * m + 1
        entry["events"] = int(ev_cnt.item())
        entry["event_capacity"] = cap
        # bytes by the algorithm: A reads 1 and writes 16 + 4 per position, a pass of B reads 1 and writes 4
        entry["A_bytes"] = 21 * n_pos
        entry["B_bytes"] = (3 * m + 1) * 5 * n_pos
        ctx.scan_dev(mo, codes.data_ptr(), None, _lib.PROFILE_NONE, n_pos, scores.data_ptr(), None, stream)
        route_a()
        torch.cuda.synchronize()
        entry["ref_column_equals_max_of_scan"] = ref_column_check(torch, codes, best, scores, m, min(n_pos, 20 * (L + 1) * 100))
        res["width_%d" % m] = entry
        mo.close()
    # ---- variants x library
    m, n_var, n_mo = 12, args.variants, args.motifs
    tables = np.stack([pssm_table(rng, m) for _ in range(n_mo)])
    var_pos = torch.randint(0, n_pos, (n_var,), dtype=torch.int64, device=dev, generator=g)
    var_alt = torch.randint(0, 4, (n_var,), dtype=torch.uint8, device=dev, generator=g)
    outs = [torch.empty((n_var, n_mo), dtype=torch.float32, device=dev) for _ in range(2)] + \
           [torch.empty((n_var, n_mo), dtype=torch.int8, device=dev) for _ in range(2)]

    def variants():
        ctx.variants_dev(tables, codes.data_ptr(), n_pos, var_pos.data_ptr(), var_alt.data_ptr(), n_var, *([o.data_ptr() for o in outs] + [stream]))

    times = timed_alternating({"variants_dev": variants}, args.iters, args.warmup)
    entry = spread(times["variants_dev"])
    entry.update({"variants": n_var, "motifs": n_mo, "width": m})
    mo = ctx.motif(tables[3])                                   # one motif's column against its dense map
    ctx.mutmap_dev(mo, codes.data_ptr(), n_pos, best.data_ptr(), where.data_ptr(), stream)
    torch.cuda.synchronize()
    ok = codes[var_pos] < 4
    want_alt = best[var_pos, var_alt.long().clamp(max=3)]
    got_alt = outs[1][:, 3]
    same = (got_alt.view(torch.int32) == want_alt.view(torch.int32)) | (torch.isnan(got_alt) & torch.isnan(want_alt))
    entry["alt_equals_dense_map_of_motif_3"] = bool(same[ok].all())
    mo.close()
    res["variants_x_library"] = entry
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
