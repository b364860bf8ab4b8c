"""Measurements of the threshold-free mutagenesis at C2 size (100k records x 3 kb, codes made on the device), the
routes taking turns inside every repetition IN THE SAME JOB:

  route L   `pfmscan_mutocc_dev`: the map of the four letters, with the occupancy (every call of the family runs it first);
  route E   `pfmscan_mutocc_events_dev` at frac = 0.5: only the gain / loss events are stored;
  route M   `pfmscan_mutmap_dev` without `where`, a log-odds table of the same width on the same codes: the sibling with the same
            count of operations (additions there, products here), float32 rows out;
  route C   `pfmscan_footprint_dev` in ratio mode, cover only: the part of the work that existed before (the ref column);
  route O   the plain `pfmscan_occupancy_dev`, which routes L, E and C run first inside the call.

for 1 motif of w = 8 and 1 motif of w = 12, each 5 times after 2 warm-ups: medians and the spread (min, max).  All run on the
context's own stream; a call is timed by the host clock from before the enqueue to the return of `pfmscan_synchronize`.  The
route the map replaces -- 3 L `occupancy` runs on mutated FASTA files per record -- is not timed: it is 3 L whole passes.  At
the size timed the map's ref column is compared with route C's cover, and the events with the filter of the map (a count and a
checksum, not a test).  Run it under `rocprofv3 --kernel-trace --stats` for kernel times, and under `--pmc` in a run of its own
for counters.

    python tools/mutocc_ab.py [--records 100000] [--length 3000] [--widths 8,12] [--iters 5] [--warmup 2] [--frac 0.5] [--out FILE]
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
    ap.add_argument("--widths", default="8,12")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frac", type=float, default=0.5)
    ap.add_argument("--capacity", type=int, default=1 << 26, help="event slots of route E")
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
    local = torch.zeros((1, n_pos, 4), dtype=torch.float64, device=dev)
    cover = torch.zeros((1, n_pos), dtype=torch.float64, device=dev)
    best = torch.empty((n_pos, 4), dtype=torch.float32, device=dev)
    occ = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
    occ_o = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
    cap = args.capacity
    ev_key = torch.empty(cap, dtype=torch.int64, device=dev)
    ev_alt = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_ref = torch.empty(cap, dtype=torch.float64, device=dev)
    ev_count = torch.zeros(1, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "frac": args.frac,
           "tile": _lib.MUTOCC_TILE, "device": ctx.device_info()}
    table = (codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec)
    for m in [int(x) for x in args.widths.split(",")]:
        T, R = tables(rng, m)
        mo = ctx.motif(T)
        torch.cuda.synchronize()

        def route_l():
            ctx.mutocc_dev(R, *table, local.data_ptr(), occ.data_ptr(), windows.data_ptr())

        def route_e():
            ev_count.zero_()
            torch.cuda.synchronize()                               # the counter is zeroed on torch's stream, the call runs on the context's
            ctx.mutocc_events_dev(R, *table, args.frac, cap, ev_key.data_ptr(), ev_alt.data_ptr(), ev_ref.data_ptr(), ev_count.data_ptr(),
                                  occ.data_ptr(), windows.data_ptr())

        def route_m():
            ctx.mutmap_dev(mo, codes.data_ptr(), n_pos, best.data_ptr(), None, None)

        def route_c():
            ctx.footprint_dev(R, None, _lib.EXPECT_RATIO, codes.data_ptr(), None, n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, None,
                              cover.data_ptr(), occ_o.data_ptr(), windows.data_ptr())

        def route_o():
            ctx.occupancy_dev(R, 4, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, occ_o.data_ptr(), windows.data_ptr())

        calls = {"L_mutocc_dev": route_l, "E_mutocc_events_dev": route_e, "M_mutmap_dev": route_m, "C_footprint_dev_ratio_cover": route_c,
                 "O_occupancy_dev": route_o}
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry["width"] = m
        o_ms = entry["O_occupancy_dev"]["median_ms"]
        for name in ("L_mutocc_dev", "E_mutocc_events_dev"):
            entry[name[0] + "_over_M"] = entry[name]["median_ms"] / entry["M_mutmap_dev"]["median_ms"]
            entry[name[0] + "_minus_O_over_M"] = (entry[name]["median_ms"] - o_ms) / entry["M_mutmap_dev"]["median_ms"]
            entry[name[0] + "_over_C"] = entry[name]["median_ms"] / entry["C_footprint_dev_ratio_cover"]["median_ms"]
        # by the algorithm: the map reads every code once and writes four doubles per position; about 2.5 m^2 products and 4 m
        # additions per position
        inside = n_rec * L
        entry["map_floor_bytes"] = inside * 33
        entry["fp64_ops"] = inside * (2.5 * m * m + 4 * m)
        entry["L_minus_O_Tops"] = entry["fp64_ops"] / max(entry["L_mutocc_dev"]["median_ms"] - o_ms, 1e-9) / 1e9
        # at the size timed: the ref column against route C's cover, the events against the filter of the map
        route_l()
        route_c()
        route_e()
        ctx.synchronize()
        c = codes.long().clamp(max=3)
        ref = local[0].gather(1, c[:, None])[:, 0]
        ok = codes < 4
        entry["ref_column_equals_footprint_cover"] = bool((ref.view(torch.int64)[ok] == cover[0].view(torch.int64)[ok]).all())
        rec = torch.arange(n_pos, device=dev) // (L + 1)
        lim = args.frac * occ[:, 0][rec]
        delta = local[0] - ref[:, None]
        mask = ((delta > lim[:, None]) | (delta < -lim[:, None])) & ok[:, None]
        n_ev = int(ev_count.cpu()[0])
        entry["events"] = n_ev
        entry["events_share_of_changes"] = n_ev / float(3 * inside)
        entry["events_equal_filter_count"] = bool(int(mask.sum()) == n_ev)
        if n_ev <= cap:
            entry["events_alt_checksum_equal"] = bool(ev_alt[:n_ev].view(torch.int64).sum() == local[0][mask].view(torch.int64).sum())
        entry["occupancy_equals_occupancy_dev"] = bool((occ.view(torch.int64) == occ_o.view(torch.int64)).all())
        res["w%d" % m] = entry
        del ref, delta, mask, lim, rec, c, ok
        mo.close()
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
