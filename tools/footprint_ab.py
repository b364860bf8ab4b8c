"""Measurements of the posterior site map at C2 size (100k records x 3 kb, codes made on the device), the routes
taking turns inside every repetition IN THE SAME JOB:

  route M   `pfmscan_footprint_dev`, both planes (start and cover), posterior weights;
  route C   `pfmscan_footprint_dev`, cover only;
  route E   `pfmscan_footprint_events_dev` at T = 0.5: only the positions with cover > T are stored;
  route X   `pfmscan_expect_dev` with posterior weights and the occupancy on the same stream and table: the part of the work
            that existed before (the occupancy pass, the inverse, a level 0 that makes every weight) -- the yardstick;
  route O   the plain `pfmscan_occupancy_dev`, which every route above runs first inside the call.

for 1 motif of w = 8 and 1 motif of w = 12, each 5 times after 2 warm-ups: medians and the spread (min, max).  All run on the
context's own stream; a call is timed by the host clock from before the enqueue to the return of `pfmscan_synchronize`.  The byte
floor of route M is stated beside the times: 1 B read + 16 B written per position and motif.  At the size timed the events are
compared with the filter of route M's planes (a count and a checksum, not a test).  Run it under `rocprofv3 --kernel-trace
--stats` for kernel times, and under `--pmc` in a run of its own for counters.

    python tools/footprint_ab.py [--records 100000] [--length 3000] [--cases 8:1,12:1] [--iters 5] [--warmup 2] [--out FILE]
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
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "threshold": args.threshold,
           "slots": _lib.FOOTPRINT_SLOTS, "device": ctx.device_info()}
    cap = args.capacity
    ev_key = torch.empty(cap, dtype=torch.int64, device=dev)
    ev_cover = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_start = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_count = torch.zeros(1, dtype=torch.int64, device=dev)
    for case in args.cases.split(","):
        m, n_mo = (int(x) for x in case.split(":"))
        R = np.stack([tables(rng, m)[1] for _ in range(n_mo)])
        start = torch.zeros((n_mo, n_pos), dtype=torch.float64, device=dev)
        cover = torch.zeros((n_mo, n_pos), dtype=torch.float64, device=dev)
        exp = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
        occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        occ_o = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        table = (codes.data_ptr(), None, n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec)

        def maps(with_start):
            ctx.footprint_dev(R, None, _lib.EXPECT_POSTERIOR, *table, start.data_ptr() if with_start else None, cover.data_ptr(), occ.data_ptr(),
                              windows.data_ptr())

        def events():
            ev_count.zero_()
            torch.cuda.synchronize()                               # the counter is zeroed on torch's stream, the call runs on the context's
            ctx.footprint_events_dev(R, None, _lib.EXPECT_POSTERIOR, *table, args.threshold, cap, ev_key.data_ptr(), ev_cover.data_ptr(),
                                     ev_start.data_ptr(), ev_count.data_ptr(), occ.data_ptr(), windows.data_ptr())

        def route_x():
            ctx.expect_dev(R, 4, _lib.EXPECT_POSTERIOR, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, exp.data_ptr(),
                           occ.data_ptr(), windows.data_ptr())

        def route_o():
            ctx.occupancy_dev(R, 4, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, occ_o.data_ptr(), windows.data_ptr())

        calls = {"M_footprint_dev_both_planes": lambda: maps(True), "C_footprint_dev_cover_only": lambda: maps(False),
                 "E_footprint_events_dev": events, "X_expect_dev_posterior": route_x, "O_occupancy_dev": route_o}
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry.update({"width": m, "motifs": n_mo})
        yard = entry["X_expect_dev_posterior"]["median_ms"]
        for name in ("M_footprint_dev_both_planes", "C_footprint_dev_cover_only", "E_footprint_events_dev"):
            entry[name[0] + "_over_X"] = entry[name]["median_ms"] / yard
            entry[name[0] + "_minus_O_ms"] = entry[name]["median_ms"] - entry["O_occupancy_dev"]["median_ms"]
        # by the algorithm: the maps form reads every code once and writes two doubles per position and motif
        inside = n_rec * L
        entry["map_floor_bytes"] = inside * n_mo * 17
        entry["M_minus_O_GBps_of_floor"] = entry["map_floor_bytes"] / max(entry["M_minus_O_ms"], 1e-9) / 1e6
        tile = _lib.FOOTPRINT_SLOTS - (m - 1)
        entry["tile_positions"] = tile
        entry["halo_share_of_chains"] = (m - 1) * -(-L // tile) / float(L + (m - 1) * -(-L // tile))
        # the events at the size timed against the filter of the planes
        maps(True)
        events()
        ctx.synchronize()
        n_ev = int(ev_count.cpu()[0])
        mask = cover > args.threshold
        entry["events"] = n_ev
        entry["events_share_of_positions"] = n_ev / float(inside * n_mo)
        entry["events_equal_filter_count"] = bool(int(mask.sum()) == n_ev)
        if n_ev <= cap:
            entry["events_cover_checksum_equal"] = bool(ev_cover[:n_ev].view(torch.int64).sum() == cover[mask].view(torch.int64).sum())
        route_o()
        ctx.synchronize()
        entry["occupancy_equals_occupancy_dev"] = bool((occ.view(torch.int64) == occ_o.view(torch.int64)).all())
        entry["max_cover"] = float(cover.max())
        res["w%d_x%d" % (m, n_mo)] = entry
        del start, cover, exp, occ, occ_o, mask
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
