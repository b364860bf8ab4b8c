"""Measurements of the multi-site model on averaged-structure profiles (DESIGN 5n "on averaged-structure profiles") at C3 size
(100k records x 3 kb, float32 rows and codes made on the device), the routes taking turns inside every repetition IN THE SAME
JOB.  Per width, one motif, lam = prior / (L - m + 1) per record (the command's default), structure only (S) and joint (J):

  route P   `pfmscan_multisite_profile_dev`, both planes (start and cover), z, nsites and windows;
  route Q   `pfmscan_multisite_profile_events_dev` at T = 0.5;
  route M   `pfmscan_footprint_profile_dev`, posterior weights and both planes, on the same rows, codes and tables: it makes the
            same chains -- a yardstick that existed before;
and once per width, on the codes of the same stream as a letter stream of the same shape and the sequence table:
  route L   `pfmscan_multisite_dev`, both planes: the two serial walks and the cover kernel that route P reuses as they are;
  route F   `pfmscan_footprint_dev`, posterior weights and both planes.

The estimate by composition is M + L - F (the chains on profile rows, plus what the multi-site model costs over the one-site
map on letters); `P_over_estimate` is the measured ratio, not a threshold.  5 whole calls after 2 warm-ups: medians and the
spread (min, max).  All run on the context's own stream; a call is timed by the host clock from before the enqueue to the return
of `pfmscan_synchronize`.  Route Q's time also holds what its protocol asks of a caller -- the event counter zeroed (on torch's
stream) and a synchronise before the call.  `--records 4096` is the batch of the command.  Run it under `rocprofv3
--kernel-trace --stats` (no counters with it) for the kernels' shares.

    python tools/multisite_profile_ab.py [--records 100000] [--length 3000] [--widths 8,12,18] [--iters 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occupancy_profile_ab import seq_table, spread, struct_tables, timed_alternating  # noqa: E402  (tools/ is the script's own directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--widths", default="8,12,18")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prior-sites", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--capacity", type=int, default=1 << 24, help="event slots of route Q")
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
    prof = torch.rand((n_pos, 7), dtype=torch.float32, device=dev, generator=g)
    prof /= prof.sum(dim=1, keepdim=True)
    rec_off = torch.arange(n_rec, dtype=torch.int64, device=dev) * (L + 1)
    rec_len = torch.full((n_rec,), L, dtype=torch.int64, device=dev)
    windows = torch.empty(n_rec, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "rows": "float32", "iters": args.iters, "warmup": args.warmup,
           "prior_sites": args.prior_sites, "threshold": args.threshold, "slots": _lib.MULTISITE_SLOTS, "chunk": _lib.MULTISITE_CHUNK,
           "library": os.path.basename(_lib.LIB_PATH), "device": ctx.device_info()}
    cap = args.capacity
    ev_key = torch.empty(cap, dtype=torch.int64, device=dev)
    ev_cover = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_start = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_count = torch.zeros(1, dtype=torch.int64, device=dev)
    start = torch.zeros((1, n_pos), dtype=torch.float64, device=dev)
    cover = torch.zeros((1, n_pos), dtype=torch.float64, device=dev)
    z = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
    ns = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
    occ = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
    for m in (int(x) for x in args.widths.split(",")):
        S = struct_tables(rng, m)[1][None]
        R = seq_table(rng, m)[None]
        lam = torch.full((n_rec,), args.prior_sites / max(L - m + 1, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        stream = (prof.data_ptr(), _lib.PROFILE_F32, n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec)
        letters = (codes.data_ptr(), None, n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec)

        def route_p(sq):
            ctx.multisite_profile_dev(S, sq, codes.data_ptr(), *stream, lam.data_ptr(), start.data_ptr(), cover.data_ptr(), z.data_ptr(),
                                      ns.data_ptr(), windows.data_ptr())

        def route_q(sq):
            ev_count.zero_()
            torch.cuda.synchronize()                               # the counter is zeroed on torch's stream, the call runs on the context's
            ctx.multisite_profile_events_dev(S, sq, codes.data_ptr(), *stream, lam.data_ptr(), args.threshold, cap, ev_key.data_ptr(),
                                             ev_cover.data_ptr(), ev_start.data_ptr(), ev_count.data_ptr(), z.data_ptr(), ns.data_ptr(),
                                             windows.data_ptr())

        def route_m(sq):
            ctx.footprint_profile_dev(S, sq, _lib.EXPECT_POSTERIOR, codes.data_ptr(), *stream, start.data_ptr(), cover.data_ptr(), occ.data_ptr(),
                                      windows.data_ptr())

        def route_l():
            ctx.multisite_dev(R, None, *letters, lam.data_ptr(), start.data_ptr(), cover.data_ptr(), z.data_ptr(), ns.data_ptr(), windows.data_ptr())

        def route_f():
            ctx.footprint_dev(R, None, _lib.EXPECT_POSTERIOR, *letters, start.data_ptr(), cover.data_ptr(), occ.data_ptr(), windows.data_ptr())

        calls = {}
        for form, sq in (("S", None), ("J", R)):
            calls[form + "_P_multisite_profile_dev_both_planes"] = lambda sq=sq: route_p(sq)
            calls[form + "_Q_multisite_profile_events_dev"] = lambda sq=sq: route_q(sq)
            calls[form + "_M_footprint_profile_dev_both_planes"] = lambda sq=sq: route_m(sq)
        calls["L_multisite_dev_both_planes"] = route_l
        calls["F_footprint_dev_both_planes"] = route_f
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry["width"] = m
        med = lambda name: entry[name]["median_ms"]   # noqa: E731
        inside = n_rec * L
        # by the algorithm: a float32 row read; plane A written, read twice; plane G written, read, written, read; two planes written
        entry["floor_bytes"] = inside * (28 + 7 * 8 + 16)
        for form, sq in (("S", None), ("J", R)):
            est = med(form + "_M_footprint_profile_dev_both_planes") + med("L_multisite_dev_both_planes") - med("F_footprint_dev_both_planes")
            entry[form + "_estimate_M_plus_L_minus_F_ms"] = est
            entry[form + "_P_over_estimate"] = med(form + "_P_multisite_profile_dev_both_planes") / est
            entry[form + "_Q_over_estimate"] = med(form + "_Q_multisite_profile_events_dev") / est
            entry[form + "_P_over_M"] = med(form + "_P_multisite_profile_dev_both_planes") / med(form + "_M_footprint_profile_dev_both_planes")
            entry[form + "_P_over_L"] = med(form + "_P_multisite_profile_dev_both_planes") / med("L_multisite_dev_both_planes")
            entry[form + "_P_GBps_of_floor"] = entry["floor_bytes"] / max(med(form + "_P_multisite_profile_dev_both_planes"), 1e-9) / 1e6
            # what came out, at the size timed (a summary, not a test)
            route_p(sq)
            route_q(sq)
            ctx.synchronize()
            n_ev = int(ev_count.cpu()[0])
            entry[form + "_events"] = n_ev
            entry[form + "_events_equal_filter_count"] = bool(int((cover > args.threshold).sum()) == n_ev)
            entry[form + "_z_median"], entry[form + "_z_max"] = float(z.median()), float(z.max())
            entry[form + "_nsites_mean"], entry[form + "_max_cover"] = float(ns.mean()), float(cover.max())
        res["w%d" % m] = entry
        del lam
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
