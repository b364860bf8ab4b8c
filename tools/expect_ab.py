"""Measurements of the expected-counts entry point at C2 size (100k records x 3 kb, codes made on the device), the
routes taking turns inside every repetition IN THE SAME JOB:

  route R   `pfmscan_expect_dev` in PFMSCAN_EXPECT_RATIO mode, with the occupancy and Windows asked for;
  route P   `pfmscan_expect_dev` in PFMSCAN_EXPECT_POSTERIOR mode, the same outputs;
  route O   `pfmscan_occupancy_dev` on the same stream and table: the part of the work that existed before, which both
            routes above run first inside the call -- the floor for them.

for 1 motif of w = 8 and 1 motif of w = 12, each 5 times after 2 warm-ups: medians and the spread (min, max).  All three run
on the context's own stream; a call is timed by the host clock from before the enqueue to the return of
`pfmscan_synchronize`.  At the size timed the occupancy that route P returns is compared bit for bit with route O's, and the
letter sums of every column of route P with 1 (a difference, not a check).  Run it under `rocprofv3 --kernel-trace --stats`
for kernel times, and under `--pmc` in a run of its own for counters.

    python tools/expect_ab.py [--records 100000] [--length 3000] [--cases 8:1,12:1] [--iters 5] [--warmup 2] [--out FILE]
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
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "device": ctx.device_info()}
    for case in args.cases.split(","):
        m, n_mo = (int(x) for x in case.split(":"))
        R = np.stack([tables(rng, m)[1] for _ in range(n_mo)])
        exp = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
        occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        occ_o = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def expect(mode):
            ctx.expect_dev(R, 4, mode, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, exp.data_ptr(), occ.data_ptr(),
                           windows.data_ptr())

        def route_o():
            ctx.occupancy_dev(R, 4, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, occ_o.data_ptr(), windows.data_ptr())

        calls = {"R_expect_dev_ratio": lambda: expect(_lib.EXPECT_RATIO), "P_expect_dev_posterior": lambda: expect(_lib.EXPECT_POSTERIOR),
                 "O_occupancy_dev": route_o}
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry.update({"width": m, "motifs": n_mo})
        floor = entry["O_occupancy_dev"]["median_ms"]
        entry["R_over_O"] = entry["R_expect_dev_ratio"]["median_ms"] / floor
        entry["P_over_O"] = entry["P_expect_dev_posterior"]["median_ms"] / floor
        # by the algorithm, per window and motif: the chain's m - 1 fp64 multiplies (made twice: once by the occupancy pass,
        # once by level 0) against 4 m fp64 additions with a select each; level 0 writes 4 m doubles per block of 32 windows
        n_win = n_rec * max(L - m + 1, 0)
        entry["chain_fp64_multiplies"] = 2 * n_win * max(m - 1, 0) * n_mo
        entry["fp64_additions_with_select"] = n_win * 4 * m * n_mo
        entry["block_sum_bytes_written"] = -(-n_win // 32) * 4 * m * n_mo * 8
        # the cells at the size timed
        route_o()
        expect(_lib.EXPECT_POSTERIOR)
        ctx.synchronize()
        entry["occupancy_equals_occupancy_dev"] = bool((occ.view(torch.int64) == occ_o.view(torch.int64)).all())
        entry["windows_all_counted"] = bool((windows == max(L - m + 1, 0)).all())
        entry["max_abs_diff_of_posterior_column_sums_to_1"] = float((exp[:, :, :, :4].sum(dim=3) - 1.0).abs().max())
        res["w%d_x%d" % (m, n_mo)] = entry
        del exp, occ, occ_o
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
