"""Measurements of the two-stream entry points at C2 size (100k records x 3 kb, both code streams made on the
device), the routes taking turns inside every repetition IN THE SAME JOB:

  route OP  `pfmscan_occupancy_pair_dev`: the joint occupancy of every record under every pair, with Windows;
  route OS  `pfmscan_occupancy_dev` on the sequence stream and then on the structure stream (n_letters 7) with the same
            tables: the part of the work that existed before.  It does NOT compute the same quantity (a sum of products is
            not a product of sums); it is the yardstick only.
  route EP  `pfmscan_expect_pair_dev` in PFMSCAN_EXPECT_POSTERIOR mode, both matrices, the occupancy and Windows;
  route ES  `pfmscan_expect_dev` on the sequence stream and then on the structure stream, the same mode and outputs: the
            yardstick of EP in the same sense.

for one pair of w = 8 and of w = 12 (all four routes) and 256 pairs of w = 12 (the occupancy routes), each 5 times after 2
warm-ups: medians and the spread (min, max).  All routes run on the context's own stream; a call is timed by the host clock
from before the enqueue to the return of `pfmscan_synchronize`.  At the size timed the occupancy that route EP returns is
compared bit for bit with route OP's.  Run it under `rocprofv3 --kernel-trace --stats` for kernel times, and under `--pmc` in a
run of its own for counters.

    python tools/pair_ab.py [--records 100000] [--length 3000] [--cases 8:1:e,12:1:e,12:256:o] [--iters 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occupancy_ab import spread, tables, timed_alternating  # noqa: E402  (tools/ is the script's own directory)


def struct_table(rng, m):
    """a structure ratio table as `-u -C 0.01` builds it from a random PFM over the 7 structure letters"""
    p = rng.dirichlet(np.full(7, 0.4), size=m)
    S = np.full((m, 8), np.nan)
    S[:, :7] = (p + 0.01) / 1.07 * 7.0
    return S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--cases", default="8:1:e,12:1:e,12:256:o", help="width:pairs:what (o: the occupancy routes, e: the expected counts too), comma separated")
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
        m, n_mo, what = case.split(":")
        m, n_mo = int(m), int(n_mo)
        R = np.stack([tables(rng, m)[1] for _ in range(n_mo)])
        S = np.stack([struct_table(rng, m) for _ in range(n_mo)])
        occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        occ_b = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def route_op():
            ctx.occupancy_pair_dev(R, S, p(codes), p(codes2), n_pos, p(rec_off), p(rec_len), n_rec, p(occ), p(windows))

        def route_os():
            ctx.occupancy_dev(R, 4, p(codes), n_pos, p(rec_off), p(rec_len), n_rec, p(occ_b), p(windows))
            ctx.occupancy_dev(S, 7, p(codes2), n_pos, p(rec_off), p(rec_len), n_rec, p(occ_b), p(windows))

        calls = {"OP_occupancy_pair_dev": route_op, "OS_two_occupancy_dev": route_os}
        if what == "e":
            e_seq = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
            e_struct = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)

            def route_ep():
                ctx.expect_pair_dev(R, S, _lib.EXPECT_POSTERIOR, p(codes), p(codes2), n_pos, p(rec_off), p(rec_len), n_rec, p(e_seq), p(e_struct),
                                    p(occ_b), p(windows))

            def route_es():
                ctx.expect_dev(R, 4, _lib.EXPECT_POSTERIOR, p(codes), n_pos, p(rec_off), p(rec_len), n_rec, p(e_seq), p(occ_b), p(windows))
                ctx.expect_dev(S, 7, _lib.EXPECT_POSTERIOR, p(codes2), n_pos, p(rec_off), p(rec_len), n_rec, p(e_struct), p(occ_b), p(windows))

            calls.update({"EP_expect_pair_dev": route_ep, "ES_two_expect_dev": route_es})
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry.update({"width": m, "pairs": n_mo})
        entry["OP_over_OS"] = entry["OP_occupancy_pair_dev"]["median_ms"] / entry["OS_two_occupancy_dev"]["median_ms"]
        n_win = n_rec * max(L - m + 1, 0)
        entry["OP_fp64_multiplies"] = n_win * (2 * m - 1) * n_mo
        entry["OP_lds_lookup_bytes"] = n_win * 2 * m * n_mo * 8
        route_op()
        ctx.synchronize()
        entry["windows_all_counted"] = bool((windows == max(L - m + 1, 0)).all())
        if what == "e":
            entry["EP_over_ES"] = entry["EP_expect_pair_dev"]["median_ms"] / entry["ES_two_expect_dev"]["median_ms"]
            route_ep()
            ctx.synchronize()
            entry["expect_occupancy_equals_occupancy_pair_dev"] = bool((occ.view(torch.int64) == occ_b.view(torch.int64)).all())
            entry["max_abs_diff_of_posterior_column_sums_to_1"] = float(max((e_seq[:, :, :, :4].sum(dim=3) - 1.0).abs().max(),
                                                                            (e_struct[:, :, :, :7].sum(dim=3) - 1.0).abs().max()))
            del e_seq, e_struct
        res["w%d_x%d" % (m, n_mo)] = entry
        del occ, occ_b
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
