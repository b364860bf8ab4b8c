"""Measurements of the occupancy on averaged-structure profiles at C3 size (100k records x 3 kb, rows and codes
made on the device), the routes taking turns inside every repetition IN THE SAME JOB:

  route A   `pfmscan_occupancy_profile_dev`, structure only: every record x motif cell in one call (the record table's
            read-back and check, the upload of the tables and the three kernels of every pass);
  route J   the same in joint mode (the letter chain over the codes first);
  route B   `pfmscan_scan_dev`'s all-scores structure pass of ONE motif on the same rows: the same reads plus a write
            stream of 8 bytes per position.  It computes another quantity (the expected log-odds); it is here as a
            kernel that is known to move these bytes well.

for 1 motif of w = 8, 12 and 18 and 256 motifs of w = 12, float32 and float64 rows, each 5 times after 2 warm-ups: medians
and the spread (min, max).  The entry point runs on the context's own stream, so every route is enqueued there and a call
is timed by the host clock from before the enqueue to the return of `pfmscan_synchronize`.  Before anything else
`tools/hbm_mixed` (built by `python -m rnascan_amd.build`) runs in the same job: its best read-only
bandwidth gives the time in which the same bytes can be read at all.  At the size timed, a column of the library call is
compared bit for bit with the single-motif call.  Run it under `rocprofv3 --kernel-trace --stats` for kernel times.

    python tools/occupancy_profile_ab.py [--records 100000] [--length 3000] [--cases 8:1,12:1,18:1,12:256] [--dtypes float32,float64]
                                         [--iters 5] [--warmup 2] [--no-floor] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def struct_tables(rng, m):
    """(structure PSSM, structure ratio table) as `-u -C 0.01` builds them from a random PFM"""
    p = rng.dirichlet(np.full(7, 0.4), size=m)
    R = (p + 0.01) / 1.07 * 7.0
    return np.log2(R), R


def seq_table(rng, m):
    p = rng.dirichlet(np.full(4, 0.4), size=m)
    R = np.full((m, 8), np.nan)
    R[:, :4] = (p + 0.01) / 1.04 / 0.25
    return R


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


def read_floor(records, length):
    """best read-only bandwidth (TB/s) of tools/hbm_mixed, and its read-only lines"""
    exe = os.path.join(REPO, "tools", "hbm_mixed")
    if not os.path.exists(exe):
        return None, ["tools/hbm_mixed is not built: NOT YET TIMED"]
    out = subprocess.run([exe, str(records), str(length)], capture_output=True, text=True, timeout=400).stdout     # the full sweep: `quick` has no read-only forms
    lines = [ln for ln in out.splitlines() if "read only" in ln]
    rates = [float(x) for ln in lines for x in re.findall(r"([0-9.]+) TB/s", ln)]
    return (max(rates) if rates else None), lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--cases", default="8:1,12:1,18:1,12:256", help="width:motifs, comma separated")
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-floor", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    floor, floor_lines = (None, ["skipped"]) if args.no_floor else read_floor(args.records, args.length)
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
    scores = torch.empty(n_pos, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "iters": args.iters, "warmup": args.warmup, "device": ctx.device_info(),
           "hbm_mixed_read_only_TBps": floor, "hbm_mixed_lines": floor_lines}
    for dtype in args.dtypes.split(","):
        tdt, code, width = (torch.float32, _lib.PROFILE_F32, 4) if dtype == "float32" else (torch.float64, _lib.PROFILE_F64, 8)
        prof = torch.rand((n_pos, 7), dtype=torch.float32, device=dev, generator=g)
        prof /= prof.sum(dim=1, keepdim=True)
        prof = prof.to(tdt)
        torch.cuda.synchronize()
        row_bytes = n_pos * 7 * width
        for case in args.cases.split(","):
            m, n_mo = (int(x) for x in case.split(":"))
            pairs = [struct_tables(rng, m) for _ in range(n_mo)]
            S = np.stack([p[1] for p in pairs])
            R = np.stack([seq_table(rng, m) for _ in range(n_mo)])
            motif = ctx.motif(None, pairs[0][0])
            occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def route_a(tabs=None, out=occ, st=S):
                ctx.occupancy_profile_dev(st, tabs, codes.data_ptr(), prof.data_ptr(), code, n_pos, rec_off.data_ptr(), rec_len.data_ptr(),
                                          n_rec, out.data_ptr(), windows.data_ptr())

            def route_b():
                ctx.scan_dev(motif, None, prof.data_ptr(), code, n_pos, None, scores.data_ptr(), None)

            calls = {"A_structure_only": route_a, "J_joint": lambda: route_a(R), "B_scan_dev_one_structure_pass": route_b}
            times = timed_alternating(ctx, calls, args.iters, args.warmup)
            entry = dict((name, spread(ms)) for name, ms in times.items())
            entry.update({"width": m, "motifs": n_mo, "rows": dtype, "row_bytes": row_bytes})
            n_win = n_rec * max(L - m + 1, 0)
            entry["A_fp64_operations"] = n_win * n_mo * (13 * m + max(m - 1, 0))          # unfused: 7 products + 6 sums per row, m - 1 products
            if floor:
                entry["read_only_ms_of_the_rows"] = row_bytes / (floor * 1e12) * 1e3
                entry["A_over_read_only"] = entry["A_structure_only"]["median_ms"] / entry["read_only_ms_of_the_rows"]
            entry["A_over_B"] = entry["A_structure_only"]["median_ms"] / entry["B_scan_dev_one_structure_pass"]["median_ms"]
            entry["J_over_A"] = entry["J_joint"]["median_ms"] / entry["A_structure_only"]["median_ms"]
            route_a()
            ctx.synchronize()
            k = min(3, n_mo - 1)
            one = torch.empty((n_rec, 1), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            route_a(None, one, S[k])
            ctx.synchronize()
            entry["column_equals_single_motif_call"] = bool((occ[:, k].contiguous().view(torch.int64) == one[:, 0].contiguous().view(torch.int64)).all())
            entry["windows_all_counted"] = bool((windows == max(L - m + 1, 0)).all())
            entry["cells_finite_and_positive"] = bool((torch.isfinite(occ) & (occ > 0)).all())
            res["%s_w%d_x%d" % (dtype, m, n_mo)] = entry
            motif.close()
            del occ, one
        del prof
        torch.cuda.empty_cache()
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
