"""Measurements of the device-side merge of the expected counts on one batch of records (4096 x 3 kb, codes made
on the host once), the two routes taking turns inside every repetition IN THE SAME JOB:

  route A   `pfmscan_expect_staged` + `expect.fsum_records` per motif: every per-record matrix comes home and is added with
            math.fsum -- the route of `--merge host`, the yardstick;
  route B   `pfmscan_expect_merged_staged` + `pfmscan_site_acc_round`: the route of `--merge device`.

and, on device buffers: `pfmscan_expect_dev` alone (E), `pfmscan_expect_merge_dev` alone over its output (M), and a plain
`torch.sum` over the same d_exp bytes (S: what only reading them costs).  Medians of 5 after 2 warm-ups and the spread; a call
is timed by the host clock from before the enqueue to the return of the synchronisation.  The matrices of route B are compared
byte for byte with route A's.  Every case runs in a process of its own under `timeout`; the first one that fails ends the run.

    python tools/expect_merge_ab.py [--records 4096] [--length 3000] [--cases 12:8,12:256] [--iters 5] [--warmup 2]
                                    [--limit 600] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occupancy_ab import spread, tables  # noqa: E402  (tools/ is the script's own directory)


def alternating(calls, sync, iters, warmup):
    for _ in range(warmup):
        for call in calls.values():
            call()
    sync()
    times = dict((name, []) for name in calls)
    for _ in range(iters):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            sync()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def one_case(args, m, n_mo):
    import torch
    from rnascan_amd import _lib, expect
    n_rec, L = args.records, args.length
    rng = np.random.default_rng(2)
    codes = rng.integers(0, 4, size=(n_rec, L + 1), dtype=np.uint8)
    codes[:, L] = 7
    codes = codes.reshape(-1)
    off = np.arange(n_rec, dtype=np.int64) * (L + 1)
    lens = np.full(n_rec, L, dtype=np.int64)
    R = np.stack([tables(rng, m)[1] for _ in range(n_mo)])
    ctx = _lib.Context(0)
    ctx.stage(codes)
    keep = {}

    def route_a():
        e, _, _ = ctx.expect_staged(R, 4, _lib.EXPECT_POSTERIOR, off, lens)
        keep["a"] = np.stack([expect.fsum_records([e[:, k]]) for k in range(n_mo)])

    def route_b():
        acc = expect.new_acc(n_mo, m)
        keep["bad"] = ctx.expect_merged_staged(R, 4, _lib.EXPECT_POSTERIOR, off, lens, acc)[0]
        keep["b"] = _lib.site_acc_round(acc).reshape(n_mo, m, 8)

    times = alternating({"A_staged_fsum": route_a, "B_merged_staged_round": route_b}, lambda: None, args.iters, args.warmup)
    entry = dict((name, spread(ms)) for name, ms in times.items())
    entry.update({"width": m, "motifs": n_mo, "records": n_rec, "length": L,
                  "same_bytes": keep["a"].tobytes() == keep["b"].tobytes(), "bad_none": bool((keep["bad"] == -1).all()),
                  "matrix_bytes": n_rec * n_mo * m * 8 * 8, "accumulator_bytes": n_mo * _lib.SITE_LIMBS * m * 8 * 8})
    entry["A_over_B"] = entry["A_staged_fsum"]["median_ms"] / entry["B_merged_staged_round"]["median_ms"]
    # the kernels on device buffers
    dev = torch.device("cuda", 0)
    d_codes = torch.from_numpy(codes).to(dev)
    d_off, d_len = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
    d_exp = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
    d_acc = torch.zeros((n_mo, _lib.SITE_LIMBS, m * 8), dtype=torch.int64, device=dev)
    d_bad = torch.zeros((n_mo, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    calls = {"E_expect_dev": lambda: ctx.expect_dev(R, 4, _lib.EXPECT_POSTERIOR, d_codes.data_ptr(), codes.size, d_off.data_ptr(), d_len.data_ptr(),
                                                    n_rec, d_exp.data_ptr()),
             "M_expect_merge_dev": lambda: ctx.expect_merge_dev(d_exp.data_ptr(), n_rec, n_mo, m, 1, d_acc.data_ptr(), d_bad.data_ptr()),
             "S_torch_sum_of_d_exp": lambda: d_exp.sum()}
    times = alternating(calls, sync, args.iters, args.warmup)
    entry.update(dict((name, spread(ms)) for name, ms in times.items()))
    e_ms, m_ms = entry["E_expect_dev"]["median_ms"], entry["M_expect_merge_dev"]["median_ms"]
    entry["merge_share_of_expect_plus_merge"] = m_ms / (e_ms + m_ms)
    entry["merge_read_TB_per_s"] = entry["matrix_bytes"] / (m_ms * 1e-3) / 1e12
    entry["device_limbs_equal_route_b"] = _lib.site_acc_round(d_acc.cpu().numpy().view(np.uint64)).reshape(n_mo, m, 8).tobytes() == keep["b"].tobytes()
    entry["device"] = ctx.device_info()
    ctx.close()
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--cases", default="12:8,12:256", help="width:motifs, comma separated")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600, help="seconds a case may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        m, n_mo = (int(x) for x in args.child.split(":"))
        print(json.dumps(one_case(args, m, n_mo)))
        return 0
    res = {}
    for case in args.cases.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", case, "--records", str(args.records),
               "--length", str(args.length), "--iters", str(args.iters), "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:                                          # nothing more is started on the device after a failure
            print("case %s ended with status %d" % (case, done.returncode), file=sys.stderr)
            return done.returncode
        res["w%s_x%s" % tuple(case.split(":"))] = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
