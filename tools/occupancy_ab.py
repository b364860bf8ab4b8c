"""Measurements of the occupancy entry point at C2 size (100k records x 3 kb, codes made on the device), the
routes taking turns inside every repetition IN THE SAME JOB:

  route A   `pfmscan_occupancy_dev`: every record x motif cell in one call (the record table's read-back and check, the
            upload of the tables and the three kernels of every pass);
  route B   the n_motifs `pfmscan_scan_dev` all-scores passes ALONE, on the same codes -- a lower bound of today's route,
            which must also bring the scores home, take exp2 and sum.

for 1 motif of w = 8, 1 motif of w = 12 and 256 motifs of w = 12, each 5 times after 2 warm-ups: medians and the spread
(min, max).  `pfmscan_occupancy_dev` runs on the context's own stream and takes no other, so both routes are enqueued there
and a call is timed by the host clock from before the enqueue to the return of `pfmscan_synchronize` (calls of milliseconds:
the clock's share is microseconds).  At the size timed, motif 3's column of the library call is compared bit for bit with
the single-motif call, and the cells with the sum of exp2 of the float32 scores (a relative difference, not a check).  Run it
under `rocprofv3 --kernel-trace --stats` for kernel times, and under `--pmc` in a run of its own for counters.

    python tools/occupancy_ab.py [--records 100000] [--length 3000] [--cases 8:1,12:1,12:256] [--iters 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tables(rng, m):
    """(log-odds table, ratio table) as `-u -C 0.01` builds them from a random PFM: ratio = (p + c) / (1 + 4 c) / 0.25"""
    p = rng.dirichlet(np.full(4, 0.4), size=m)
    R = np.full((m, 8), np.nan)
    R[:, :4] = (p + 0.01) / 1.04 / 0.25
    T = np.full((m, 8), np.nan)
    T[:, :4] = np.log2(R[:, :4])
    return T, R


def timed_alternating(ctx, calls, iters, warmup):
    """{name: [ms]}: the calls take turns inside every repetition; host clock around enqueue + synchronise of the ctx's stream"""
    for _ in range(warmup):
        for call in calls.values():
            call()
    ctx.synchronize()
    times = dict((name, []) for name in calls)
    for _ in range(iters):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--cases", default="8:1,12:1,12:256", help="width:motifs, comma separated")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
    scores = torch.empty(n_pos, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "device": ctx.device_info()}
    for case in args.cases.split(","):
        m, n_mo = (int(x) for x in case.split(":"))
        pairs = [tables(rng, m) for _ in range(n_mo)]
        R = np.stack([p[1] for p in pairs])
        motifs = [ctx.motif(p[0]) for p in pairs]
        occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def route_a():
            ctx.occupancy_dev(R, 4, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, occ.data_ptr(), windows.data_ptr())

        def route_b():
            for mo in motifs:
                ctx.scan_dev(mo, codes.data_ptr(), None, _lib.PROFILE_NONE, n_pos, scores.data_ptr(), None, None)

        times = timed_alternating(ctx, {"A_occupancy_dev": route_a, "B_scan_dev_passes_alone": route_b}, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry.update({"width": m, "motifs": n_mo, "B_passes": n_mo})
        # by the algorithm: m fp64 multiplies and m LDS look-ups of 8 bytes per window and motif; A reads the codes once per
        # pass over the records and writes 8 bytes per block sum and motif, a pass of B reads 1 and writes 4 bytes per position
        n_win = n_rec * max(L - m + 1, 0)
        entry["A_fp64_multiplies"] = n_win * max(m - 1, 0) * n_mo
        entry["A_lds_lookup_bytes"] = n_win * m * n_mo * 8
        entry["B_bytes"] = n_mo * 5 * n_pos
        # the cells at the size timed
        route_a()
        ctx.synchronize()
        k = min(3, n_mo - 1)
        one = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.occupancy_dev(R[k], 4, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, one.data_ptr(), None)
        ctx.scan_dev(motifs[k], codes.data_ptr(), None, _lib.PROFILE_NONE, n_pos, scores.data_ptr(), None, None)
        ctx.synchronize()
        entry["column_equals_single_motif_call"] = bool((occ[:, k].contiguous().view(torch.int64) == one[:, 0].contiguous().view(torch.int64)).all())
        entry["windows_all_counted"] = bool((windows == max(L - m + 1, 0)).all())
        by_exp2 = torch.exp2(torch.nan_to_num(scores.double(), nan=-float("inf"))).view(n_rec, L + 1).sum(dim=1)
        entry["max_rel_diff_to_sum_of_exp2_of_float32_scores"] = float(((occ[:, k] - by_exp2).abs() / by_exp2).max())
        res["w%d_x%d" % (m, n_mo)] = entry
        for mo in motifs:
            mo.close()
        del occ, one
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
