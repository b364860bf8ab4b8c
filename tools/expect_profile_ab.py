"""Measurements of the expected counts on averaged-structure profiles at C3 size (100k records x 3 kb, float32 rows
and codes made on the device), the routes taking turns inside every repetition IN THE SAME JOB.  Per width, one motif:

  route S   `pfmscan_expect_profile_dev`, struct_tables only (PFMSCAN_EXPECT_POSTERIOR, occ and Windows asked for);
  route J   the same with both tables (joint weights), exp_seq asked for;
  route Q   the same with seq_tables only, exp_seq asked for;
  route OS  `pfmscan_occupancy_profile_dev`, structure only, on the same stream and table: the part of route S that existed
            before, which the call runs first -- its floor;
  route OJ  `pfmscan_occupancy_profile_dev`, joint: the floor of route J;
  route OQ  `pfmscan_occupancy_dev` on the codes: the floor of route Q.

5 whole calls after 2 warm-ups: medians and the spread (min, max).  All run on the context's own stream; a call is timed by
the host clock from before the enqueue to the return of `pfmscan_synchronize`.  At the size timed the occupancy every route
returns is compared bit for bit with its floor's (a check of the measurement, not a test).  Run it under
`rocprofv3 --kernel-trace --stats` for kernel times, in a run of its own.

    python tools/expect_profile_ab.py [--records 100000] [--length 3000] [--widths 8,12,18] [--iters 5] [--warmup 2] [--out FILE]
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
           "device": ctx.device_info()}
    for m in (int(x) for x in args.widths.split(",")):
        S = struct_tables(rng, m)[1][None]
        R = seq_table(rng, m)[None]
        e_st = torch.empty((n_rec, 1, m, 8), dtype=torch.float64, device=dev)
        e_sq = torch.empty((n_rec, 1, m, 8), dtype=torch.float64, device=dev)
        occ = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
        occ_o = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def expect(st, sq):
            ctx.expect_profile_dev(st, sq, _lib.EXPECT_POSTERIOR, codes.data_ptr(), prof.data_ptr(), _lib.PROFILE_F32, n_pos, rec_off.data_ptr(),
                                   rec_len.data_ptr(), n_rec, e_st.data_ptr(), e_sq.data_ptr() if sq is not None else None, occ.data_ptr(),
                                   windows.data_ptr())

        def floor(st, sq):
            if st is None:
                ctx.occupancy_dev(sq, 4, codes.data_ptr(), n_pos, rec_off.data_ptr(), rec_len.data_ptr(), n_rec, occ_o.data_ptr(), windows.data_ptr())
            else:
                ctx.occupancy_profile_dev(st, sq, codes.data_ptr(), prof.data_ptr(), _lib.PROFILE_F32, n_pos, rec_off.data_ptr(), rec_len.data_ptr(),
                                          n_rec, occ_o.data_ptr(), windows.data_ptr())

        forms = {"S": (S, None), "J": (S, R), "Q": (None, R)}
        calls = {}
        for name, (st, sq) in forms.items():
            calls[name + "_expect_profile_dev"] = lambda st=st, sq=sq: expect(st, sq)
            calls["O" + name + "_occupancy"] = lambda st=st, sq=sq: floor(st, sq)
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry["width"] = m
        n_win = n_rec * max(L - m + 1, 0)
        # by the algorithm, per window: level 0 adds 7 m products and 7 m additions to the marginal chain's 8 m operations
        entry["level0_fp64_products"] = n_win * 7 * m
        entry["level0_fp64_additions"] = n_win * 7 * m
        entry["block_sum_bytes_written_struct"] = -(-n_win // 32) * 7 * m * 8
        for name, (st, sq) in forms.items():
            entry[name + "_over_floor"] = entry[name + "_expect_profile_dev"]["median_ms"] / entry["O" + name + "_occupancy"]["median_ms"]
            floor(st, sq)
            expect(st, sq)
            ctx.synchronize()
            entry[name + "_occupancy_equals_floor"] = bool((occ.view(torch.int64) == occ_o.view(torch.int64)).all())
            entry[name + "_all_finite"] = bool(torch.isfinite(e_st).all())
            if sq is None:                                           # posterior weights, rows that sum to 1: a matrix row sums to ~1
                entry["S_max_abs_diff_of_row_sums_to_1"] = float((e_st[:, :, :, :7].sum(dim=3) - 1.0).abs().max())
        res["w%d" % m] = entry
        del e_st, e_sq, occ, occ_o
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
