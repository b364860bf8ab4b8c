"""Measurements of the expected letter-pair table of two code streams (`pfmscan_expect_pair_joint_dev`) at C2 size
(100k records x 3 kb, both code streams made on the device), the routes taking turns inside every repetition IN THE SAME JOB:

  route EP  `pfmscan_expect_pair_dev`, both margins: the part of the call that existed before -- the yardstick;
  route JM  `pfmscan_expect_pair_joint_dev`, the table and both margins;
  route J   `pfmscan_expect_pair_joint_dev`, the table alone (both margins NULL);

all in PFMSCAN_EXPECT_POSTERIOR mode with the occupancy and Windows, for one pair of w = 8 and of w = 12 and 256 pairs of
w = 12, each 5 times after 2 warm-ups: medians and the spread (min, max).  All routes run on the context's own stream; a call is
timed by the host clock from before the enqueue to the return of `pfmscan_synchronize`.  At the size timed the margins of route
JM are compared with route EP's by the wrapping sums of their bit patterns, and the table's row and column sums with them to a
printed difference.  Run it under `rocprofv3 --kernel-trace --stats` for the level-0 kernel's share, and under `--pmc` in a run of its own for counters.
The table takes 32 m doubles per record and pair: 78.6 GB at 100k records x 256 pairs of w = 12 -- `--records` bounds it.

    python tools/pair_joint_ab.py [--records 100000] [--length 3000] [--cases 8:1,12:1,12:256] [--iters 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occupancy_ab import spread, tables, timed_alternating  # noqa: E402  (tools/ is the script's own directory)
from pair_ab import struct_table  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--cases", default="8:1,12:1,12:256", help="width:pairs, comma separated")
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
    codes2 = torch.randint(0, 7, (n_pos,), dtype=torch.uint8, device=dev, generator=g)
    codes.view(n_rec, L + 1)[:, L] = 7
    codes2.view(n_rec, L + 1)[:, L] = 7
    rec_off = torch.arange(n_rec, dtype=torch.int64, device=dev) * (L + 1)
    rec_len = torch.full((n_rec,), L, dtype=torch.int64, device=dev)
    windows = torch.empty(n_rec, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "device": ctx.device_info()}
    p = lambda t: t.data_ptr()
    for case in args.cases.split(","):
        m, n_mo = (int(x) for x in case.split(":"))
        R = np.stack([tables(rng, m)[1] for _ in range(n_mo)])
        S = np.stack([struct_table(rng, m) for _ in range(n_mo)])
        occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        e_seq = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
        e_struct = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
        e_joint = torch.empty((n_rec, n_mo, m, 4, 8), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        streams = (p(codes), p(codes2), n_pos, p(rec_off), p(rec_len), n_rec)

        def route_ep():
            ctx.expect_pair_dev(R, S, _lib.EXPECT_POSTERIOR, *streams, p(e_seq), p(e_struct), p(occ), p(windows))

        def route_jm():
            ctx.expect_pair_joint_dev(R, S, _lib.EXPECT_POSTERIOR, *streams, p(e_seq), p(e_struct), p(e_joint), p(occ), p(windows))

        def route_j():
            ctx.expect_pair_joint_dev(R, S, _lib.EXPECT_POSTERIOR, *streams, None, None, p(e_joint), p(occ), p(windows))

        times = timed_alternating(ctx, {"EP_margins": route_ep, "JM_table_and_margins": route_jm, "J_table_alone": route_j}, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry.update({"width": m, "pairs": n_mo, "table_bytes": e_joint.numel() * 8})
        entry["JM_over_EP"] = entry["JM_table_and_margins"]["median_ms"] / entry["EP_margins"]["median_ms"]
        entry["J_over_EP"] = entry["J_table_alone"]["median_ms"] / entry["EP_margins"]["median_ms"]
        bits = lambda: (int(e_seq.view(torch.int64).sum()), int(e_struct.view(torch.int64).sum()))   # wrapping sums of the bit patterns
        e_seq.fill_(-1.0)
        e_struct.fill_(-1.0)
        torch.cuda.synchronize()
        route_ep()
        ctx.synchronize()
        of_ep = bits()
        e_seq.fill_(-1.0)
        e_struct.fill_(-1.0)
        torch.cuda.synchronize()
        route_jm()
        ctx.synchronize()
        entry["margins_bit_sums_equal_expect_pair_dev"] = bits() == of_ep
        entry["max_abs_diff_of_table_rows_to_exp_seq"] = float((e_joint.sum(dim=4) - e_seq[:, :, :, :4]).abs().max())
        entry["max_abs_diff_of_table_columns_to_exp_struct"] = float((e_joint.sum(dim=3) - e_struct).abs().max())
        res["w%d_x%d" % (m, n_mo)] = entry
        del occ, e_seq, e_struct, e_joint
        torch.cuda.empty_cache()
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
