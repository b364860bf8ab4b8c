"""Cost of the joint threshold on LogOdds.SeqStruct (pfmscan_hits_sum_staged) against the plain fused hits pass, one process.

    python tools/sum_hits_ab.py [--records 100000] [--length 3000] [--widths 12 18] [--calls 50] [--hit-rate 1e-4]

A C3-size synthetic stream (bench_legs.make_stream: float32 rows) is generated on the device, copied home and staged once.
Per width, interleaved in blocks of ten calls:
  plain  hits_staged(thr_seq = -inf, thr_struct = S)             the fused hits pass as the parent has it (PFMSCAN_TWO_PHASE=0)
  sum    hits_sum_staged(thr_seq = thr_struct = -inf, T)         the same pass with the third predicate
S and T are the scores between the k-th and (k+1)-th largest, k = hit rate x windows: both calls return k hits, read the same
bytes and sort the same number of hits home.  Reported: the medians of the wall time of a call, the spread of the plain
pass (max - min of its block medians) and the verdict  median(sum) <= median(plain) + spread + 5 %.  Last, today's only
alternative: all scores home (scan_staged) and the filter on the printed sum in numpy.  One JSON line per width."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["PFMSCAN_TWO_PHASE"] = "0"          # read when the ctx is made


def kth_gap(torch, x, k):
    """a threshold between the k-th and the (k+1)-th largest value of x: `x > thr` holds for exactly k entries (no ties)"""
    top = torch.topk(x, k + 1).values
    return 0.5 * (float(top[k - 1]) + float(top[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--widths", type=int, nargs="+", default=[12, 18])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--hit-rate", type=float, default=1e-4)
    ap.add_argument("--host-filter-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    from bench_legs import make_pssms, make_stream
    from rnascan_amd import _lib
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    codes_d, profile_d, n_pos = make_stream(torch, dev, args.records, args.length, 20240601)
    codes, profile = codes_d.cpu().numpy(), profile_d.cpu().numpy()
    ctx.stage(codes, profile)
    out_seq = torch.zeros(n_pos, dtype=torch.float32, device=dev)
    out_st = torch.zeros(n_pos, dtype=torch.float64, device=dev)
    for w in args.widths:
        table, spssm = make_pssms(w, "finite")
        motif = ctx.motif(table, spssm)
        windows = args.records * (args.length - w + 1)
        k = max(1, int(round(args.hit_rate * windows)))
        ctx.scan_dev(motif, codes_d.data_ptr(), profile_d.data_ptr(), _lib.PROFILE_F32, n_pos, out_seq.data_ptr(), out_st.data_ptr(), None)
        ctx.synchronize()
        torch.cuda.synchronize()
        ok = torch.isfinite(out_seq) & torch.isfinite(out_st)
        neg = torch.full_like(out_st, -float("inf"))
        thr_struct = kth_gap(torch, torch.where(ok, out_st, neg), k)
        printed = (torch.round(out_seq * 1000.0) / 1000.0).double() + out_st          # float32 multiply, rint, divide; fp64 add
        thr_sum = kth_gap(torch, torch.where(ok, printed, neg), k)
        del ok, neg, printed
        calls = {"plain": lambda: ctx.hits_staged(motif, -np.inf, thr_struct),
                 "sum": lambda: ctx.hits_sum_staged(motif, -np.inf, -np.inf, thr_sum)}
        n_hits = {name: len(f()[0]) for name, f in calls.items()}                      # warm: kernels loaded, scratch sized
        times = {"plain": [], "sum": []}
        blocks = {"plain": [], "sum": []}
        per_block = 10
        for _ in range(max(1, args.calls // per_block)):
            for name in ("plain", "sum"):
                t = []
                for _ in range(per_block):
                    t0 = time.perf_counter()
                    calls[name]()
                    t.append((time.perf_counter() - t0) * 1e3)
                times[name] += t
                blocks[name].append(statistics.median(t))
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = max(blocks["plain"]) - min(blocks["plain"])
        allowed = med["plain"] + spread + 0.05 * med["plain"]
        host = []
        for _ in range(args.host_filter_reps):
            t0 = time.perf_counter()
            sq, st = ctx.scan_staged(motif)
            with np.errstate(invalid="ignore"):
                pos = np.flatnonzero(np.round(sq, 3).astype(np.float64) + st > thr_sum)
            host.append((time.perf_counter() - t0) * 1e3)
            n_host = int(pos.size)
            del sq, st, pos
        motif.close()
        print(json.dumps({
            "width": w, "records": args.records, "length": args.length, "windows": windows, "target_hits": k, "hits": n_hits,
            "hits_all_scores_plus_host_filter": n_host, "thr_struct": thr_struct, "thr_sum": thr_sum,
            "calls_per_pass": len(times["plain"]), "median_ms": {n: round(v, 4) for n, v in med.items()},
            "min_ms": {n: round(min(v), 4) for n, v in times.items()},
            "plain_block_medians_ms": [round(v, 4) for v in blocks["plain"]], "sum_block_medians_ms": [round(v, 4) for v in blocks["sum"]],
            "plain_spread_ms": round(spread, 4), "allowed_ms": round(allowed, 4),
            "sum_over_plain": round(med["sum"] / med["plain"], 4), "verdict": "inside" if med["sum"] <= allowed else "outside",
            "all_scores_plus_host_filter_ms": [round(v, 1) for v in host]}))
        sys.stdout.flush()
    ctx.close()


if __name__ == "__main__":
    main()
