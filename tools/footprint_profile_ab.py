"""Measurements of the posterior site map on averaged-structure profiles at C3 size (100k records x 3 kb, float32
rows and codes made on the device), the routes taking turns inside every repetition IN THE SAME JOB.  Per width, one motif,
posterior weights, the occupancy and Windows asked for, structure only (S) and joint (J):

  route M   `pfmscan_footprint_profile_dev`, both planes (start and cover);
  route C   `pfmscan_footprint_profile_dev`, cover only;
  route E   `pfmscan_footprint_profile_events_dev` at T = 0.5: only the positions with cover > T are stored;
  route O   `pfmscan_occupancy_profile_dev` on the same stream and tables: the pass every route above runs first inside the call;
  route X   `pfmscan_expect_profile_dev`, the existing call that makes the same weights (and sums them away by row).

5 whole calls after 2 warm-ups: medians and the spread (min, max).  All run on the context's own stream; a call is timed by
the host clock from before the enqueue to the return of `pfmscan_synchronize`.  Route E's time also holds what its protocol
asks of a caller -- the event counter zeroed (here on torch's stream, one small kernel) and a synchronise before the call --
which routes M and C do not pay (not measured apart): E against M compares two calls as a caller makes them, not two kernels.
The byte floor of route M is stated beside the times: 28 B read (a float32 row) + 16 B written per position and motif.  At the
size timed the events are compared with the filter of route M's planes and the occupancy with route O's (a count and a checksum: checks of the measurement, not tests).
``--slots`` only labels the result: the geometry is the library's (PFMSCAN_LIB selects a build of tools/build_variant.sh made
with -DPFMSCAN_FPP_SLOTS=512).  Run it under `rocprofv3 --kernel-trace --stats` for kernel times, and under `--pmc` in a run
of its own for counters.

    python tools/footprint_profile_ab.py [--records 100000] [--length 3000] [--widths 8,12,18,64] [--routes MCEOX] [--iters 5]
                                         [--warmup 2] [--slots N] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occupancy_profile_ab import seq_table, spread, struct_tables, timed_alternating  # noqa: E402  (tools/ is the script's own directory)

NAMES = {"M": "footprint_profile_dev_both_planes", "C": "footprint_profile_dev_cover_only", "E": "footprint_profile_events_dev",
         "O": "occupancy_profile_dev", "X": "expect_profile_dev"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--widths", default="8,12,18,64")
    ap.add_argument("--routes", default="MCEOX")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--capacity", type=int, default=1 << 24, help="event slots of route E")
    ap.add_argument("--slots", type=int, default=None, help="the geometry of the library that is loaded (a label)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib
    n_rec, L = args.records, args.length
    n_pos = n_rec * (L + 1)
    slots = args.slots or _lib.FOOTPRINT_PROFILE_SLOTS
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    codes = torch.randint(0, 4, (n_pos,), dtype=torch.uint8, device=dev, generator=g)
    codes.view(n_rec, L + 1)[:, L] = 7
    prof = torch.rand((n_pos, 7), dtype=torch.float32, device=dev, generator=g)
    prof /= prof.sum(dim=1, keepdim=True)
    rec_off = torch.arange(n_rec, dtype=torch.int64, device=dev) * (L + 1)
    rec_len = torch.full((n_rec,), L, dtype=torch.int64, device=dev)
    windows = torch.empty(n_rec, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "rows": "float32", "iters": args.iters, "warmup": args.warmup,
           "threshold": args.threshold, "slots": slots, "library": os.path.basename(_lib.LIB_PATH), "device": ctx.device_info()}
    cap = args.capacity
    ev_key = torch.empty(cap, dtype=torch.int64, device=dev)
    ev_cover = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_start = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_count = torch.zeros(1, dtype=torch.int64, device=dev)
    start = torch.zeros((1, n_pos), dtype=torch.float64, device=dev)
    cover = torch.zeros((1, n_pos), dtype=torch.float64, device=dev)
    occ = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
    occ_o = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
    for m in (int(x) for x in args.widths.split(",")):
        S = struct_tables(rng, m)[1][None]
        R = seq_table(rng, m)[None]
        e_st = torch.empty((n_rec, 1, m, 8), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        stream = (prof.data_ptr(), _lib.PROFILE_F32, n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec)

        def maps(sq, with_start):
            ctx.footprint_profile_dev(S, sq, _lib.EXPECT_POSTERIOR, codes.data_ptr(), *stream, start.data_ptr() if with_start else None,
                                      cover.data_ptr(), occ.data_ptr(), windows.data_ptr())

        def events(sq):
            ev_count.zero_()
            torch.cuda.synchronize()                               # the counter is zeroed on torch's stream, the call runs on the context's
            ctx.footprint_profile_events_dev(S, sq, _lib.EXPECT_POSTERIOR, codes.data_ptr(), *stream, args.threshold, cap, ev_key.data_ptr(),
                                             ev_cover.data_ptr(), ev_start.data_ptr(), ev_count.data_ptr(), occ.data_ptr(), windows.data_ptr())

        def route_o(sq):
            ctx.occupancy_profile_dev(S, sq, codes.data_ptr(), *stream, occ_o.data_ptr(), windows.data_ptr())

        def route_x(sq):
            ctx.expect_profile_dev(S, sq, _lib.EXPECT_POSTERIOR, codes.data_ptr(), *stream, e_st.data_ptr(), None, occ.data_ptr(), windows.data_ptr())

        route = {"M": lambda sq: maps(sq, True), "C": lambda sq: maps(sq, False), "E": events, "O": route_o, "X": route_x}
        calls = {}
        for form, sq in (("S", None), ("J", R)):
            for r in args.routes:
                calls["%s_%s_%s" % (form, r, NAMES[r])] = lambda r=r, sq=sq: route[r](sq)
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry["width"] = m
        med = lambda form, r: entry["%s_%s_%s" % (form, r, NAMES[r])]["median_ms"] if r in args.routes else None   # noqa: E731
        inside = n_rec * L
        tile = slots - (m - 1)
        entry["tile_positions"] = tile
        entry["halo_share_of_chains"] = (m - 1) * -(-L // tile) / float(L + (m - 1) * -(-L // tile))
        # by the algorithm: the maps form reads every float32 row once and writes two doubles per position and motif
        entry["map_floor_bytes"] = inside * 44
        for form, sq in (("S", None), ("J", R)):
            for r in "MCE":
                if med(form, r) is None:
                    continue
                if med(form, "X") is not None:
                    entry["%s_%s_over_X" % (form, r)] = med(form, r) / med(form, "X")
                if med(form, "O") is not None:
                    entry["%s_%s_over_O" % (form, r)] = med(form, r) / med(form, "O")
                    entry["%s_%s_minus_O_ms" % (form, r)] = med(form, r) - med(form, "O")
            if med(form, "M") is not None:
                entry[form + "_M_GBps_of_floor_whole_call"] = entry["map_floor_bytes"] / med(form, "M") / 1e6
                if med(form, "O") is not None:
                    entry[form + "_M_minus_O_GBps_of_floor"] = entry["map_floor_bytes"] / max(med(form, "M") - med(form, "O"), 1e-9) / 1e6
            # the events at the size timed against the filter of the planes; the occupancy against route O's
            maps(sq, True)
            events(sq)
            route_o(sq)
            ctx.synchronize()
            n_ev = int(ev_count.cpu()[0])
            mask = cover > args.threshold
            entry[form + "_events"] = n_ev
            entry[form + "_events_share_of_positions"] = n_ev / float(inside)
            entry[form + "_events_equal_filter_count"] = bool(int(mask.sum()) == n_ev)
            if n_ev <= cap:
                entry[form + "_events_cover_checksum_equal"] = bool(ev_cover[:n_ev].view(torch.int64).sum() == cover[mask].view(torch.int64).sum())
            entry[form + "_occupancy_equals_occupancy_profile_dev"] = bool((occ.view(torch.int64) == occ_o.view(torch.int64)).all())
            entry[form + "_max_cover"] = float(cover.max())
            del mask
        res["w%d" % m] = entry
        del e_st
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
