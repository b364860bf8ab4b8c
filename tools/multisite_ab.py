"""Measurements of the multi-site model at C2 size (100k records x 3 kb, codes made on the device), the routes taking
turns inside every repetition IN THE SAME JOB:

  route S   `pfmscan_multisite_dev`, both planes (start and cover), z, nsites and windows;
  route E   `pfmscan_multisite_events_dev` at T = 0.5;
  route F   `pfmscan_footprint_dev` with posterior weights and both planes on the same stream and table: the one-site model
            that existed before -- the yardstick.

for 1 motif of w = 8 and 1 motif of w = 12, each 5 times after 2 warm-ups: medians and the spread (min, max).  All run on the
context's own stream; a call is timed by the host clock from before the enqueue to the return of `pfmscan_synchronize`.
lam = prior / (L - m + 1) per record, the command's default.  `--records 4096` is the batch of the command, where the two
serial kernels have 64 waves.  Run it under `rocprofv3 --kernel-trace --stats` for the share of the two serial kernels.

    python tools/multisite_ab.py [--records 100000] [--length 3000] [--cases 8:1,12:1] [--iters 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occupancy_ab import spread, tables, timed_alternating  # noqa: E402  (tools/ is the script's own directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--cases", default="8:1,12:1", help="width:motifs, comma separated")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prior-sites", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--capacity", type=int, default=1 << 24, help="event slots of route E")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib
    n_rec, L = args.records, args.length
    n_pos = n_rec * (L + 1)
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    codes = torch.randint(0, 4, (n_pos,), dtype=torch.uint8, device=dev, generator=g)
    codes.view(n_rec, L + 1)[:, L] = 7
    rec_off = torch.arange(n_rec, dtype=torch.int64, device=dev) * (L + 1)
    rec_len = torch.full((n_rec,), L, dtype=torch.int64, device=dev)
    windows = torch.empty(n_rec, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "prior_sites": args.prior_sites,
           "slots": _lib.MULTISITE_SLOTS, "chunk": _lib.MULTISITE_CHUNK, "device": ctx.device_info()}
    cap = args.capacity
    ev_key = torch.empty(cap, dtype=torch.int64, device=dev)
    ev_cover = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_start = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_count = torch.zeros(1, dtype=torch.int64, device=dev)
    for case in args.cases.split(","):
        m, n_mo = (int(x) for x in case.split(":"))
        R = np.stack([tables(rng, m)[1] for _ in range(n_mo)])
        lam = torch.full((n_rec,), args.prior_sites / max(L - m + 1, 1), dtype=torch.float64, device=dev)
        start = torch.zeros((n_mo, n_pos), dtype=torch.float64, device=dev)
        cover = torch.zeros((n_mo, n_pos), dtype=torch.float64, device=dev)
        z = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        ns = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        table = (codes.data_ptr(), None, n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec)

        def route_s():
            ctx.multisite_dev(R, None, *table, lam.data_ptr(), start.data_ptr(), cover.data_ptr(), z.data_ptr(), ns.data_ptr(), windows.data_ptr())

        def route_e():
            ev_count.zero_()
            torch.cuda.synchronize()                               # the counter is zeroed on torch's stream, the call runs on the context's
            ctx.multisite_events_dev(R, None, *table, lam.data_ptr(), args.threshold, cap, ev_key.data_ptr(), ev_cover.data_ptr(),
                                     ev_start.data_ptr(), ev_count.data_ptr(), z.data_ptr(), ns.data_ptr(), windows.data_ptr())

        def route_f():
            ctx.footprint_dev(R, None, _lib.EXPECT_POSTERIOR, *table, start.data_ptr(), cover.data_ptr(), occ.data_ptr(), windows.data_ptr())

        calls = {"S_multisite_dev_both_planes": route_s, "E_multisite_events_dev": route_e, "F_footprint_dev_both_planes": route_f}
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry.update({"width": m, "motifs": n_mo})
        yard = entry["F_footprint_dev_both_planes"]["median_ms"]
        for name in ("S_multisite_dev_both_planes", "E_multisite_events_dev"):
            entry[name[0] + "_over_F"] = entry[name]["median_ms"] / yard
        # by the algorithm: 1 B of codes read; plane A written, read twice; plane G written, read, written, read; two planes written
        inside = n_rec * L
        entry["floor_bytes"] = inside * n_mo * (1 + 7 * 8 + 16)
        entry["S_GBps_of_floor"] = entry["floor_bytes"] / max(entry["S_multisite_dev_both_planes"]["median_ms"], 1e-9) / 1e6
        # what came out, at the size timed (a summary, not a test)
        route_s()
        route_e()
        ctx.synchronize()
        n_ev = int(ev_count.cpu()[0])
        entry["events"] = n_ev
        entry["events_equal_filter_count"] = bool(int((cover > args.threshold).sum()) == n_ev)
        entry["z_median"], entry["z_max"] = float(z.median()), float(z.max())
        entry["nsites_mean"], entry["max_cover"] = float(ns.mean()), float(cover.max())
        res["w%d_x%d" % (m, n_mo)] = entry
        del start, cover, z, ns, occ, lam
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
