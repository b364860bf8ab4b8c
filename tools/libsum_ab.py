"""--min-seqstruct on a motif library: the joint threshold decided in the library kernel (pfmscan_library_hits_sum_staged)
against the routes it replaces, one process, interleaved in blocks, medians.

    python tools/libsum_ab.py [--records 100000] [--length 3000] [--pairs 256] [--width 12] [--blocks 5] [--sample-pairs 8]
                              [--total-hits 5e6]
    python tools/libsum_ab.py --plain-only [--repo OTHER_CHECKOUT] ...      leg (c) for one build; a job alternates the builds

C5's stream (bench_legs.make_stream: float32 rows) is generated on the device, copied home and staged once; the library is
C5's (bench_legs.make_pssms, seeds 1000 ..).  Every pair gets its own T between the k-th and (k+1)-th largest printed sum
float64(round(float32 seq, 3)) + struct of ITS windows, k = total hits / pairs.  A block is one call of each leg:
  (a) sum        library_hits_sum_staged(thr_seq = thr_struct = -inf, T)                one pass, all pairs
      per_pair   hits_sum_staged per pair at the same thresholds, the parent's only route: timed for --sample-pairs pairs
                 spread over the library and SCALED by pairs / sample (said so in the output)
  (b) plain_eff  library_hits_staged(thr_seq = thr_eff, thr_struct = -inf): the same phase-A survivors, without the predicate.
                 Its hit set is every survivor, far beyond any buffer when thr_eff is dense: it runs with a small capacity and may
                 end in PFMSCAN_E_CAPACITY (the kernel then still scores and counts every window; only the stores are skipped)
  (c) plain_c5   library_hits_staged at C5's own thresholds (-m 6, bench_legs.combined_threshold)
Beside the times: phase A's survivor rate at thr_eff BRACKETED per pair -- from below by the share of windows with
seq > thr_eff (what the credits must keep), from above by the share with seq > thr_eff - slack, slack the one-sided slack of
the pair's credit table (pfmscan_debug_credit_table: the credits keep nothing below that) -- max_eps (the largest slack), and
U_k - the largest structure score seen, for the sampled pairs.  One JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np


def kth_gap(torch, x, k):
    """a threshold between the k-th and the (k+1)-th largest value of x (no ties assumed); x = -inf where it does not count"""
    n = x.numel()
    if n > (1 << 24) and k < n // 4096:
        # a cut from a sample first: the exact order statistics are then taken among the few values above it
        step = 97
        sample = x[::step]
        ks = min(sample.numel() - 1, int(2.0 * k / step) + 64)
        cut = float(torch.topk(sample, ks + 1).values[ks])
        cand = x[x > cut]
        if cand.numel() > k:
            top = torch.topk(cand, k + 1).values
            return 0.5 * (float(top[k - 1]) + float(top[k]))
    top = torch.topk(x, k + 1).values
    return 0.5 * (float(top[k - 1]) + float(top[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--width", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--sample-pairs", type=int, default=8)
    ap.add_argument("--total-hits", type=float, default=5e6)
    ap.add_argument("--plain-only", action="store_true", help="leg (c) alone: needs nothing this build adds")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose rnascan_amd (and libpfmscan.so) is loaded")
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    from bench_legs import combined_threshold, make_pssms, make_stream, probe_motifs
    from rnascan_amd import _lib
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    w, n_lib = args.width, args.pairs
    codes_d, profile_d, n_pos = make_stream(torch, dev, args.records, args.length, 20240601)
    windows = args.records * (args.length - w + 1)
    out_seq = torch.zeros(n_pos, dtype=torch.float32, device=dev)
    out_st = torch.zeros(n_pos, dtype=torch.float64, device=dev)
    tabs = [make_pssms(w, "finite", seed=1000 + k) for k in range(n_lib)]
    LT, LP = np.stack([t for t, _ in tabs]), np.stack([p for _, p in tabs])
    motifs = [ctx.motif(*tp) for tp in probe_motifs(tabs)]
    thr_c5, rate_seq, _ = combined_threshold(torch, ctx, motifs, codes_d, profile_d, _lib.PROFILE_F32, n_pos, out_seq, out_st, None,
                                             windows, 6.0, 1e-4)
    for m0 in motifs:
        m0.close()
    result = {"label": args.label, "records": args.records, "length": args.length, "pairs": n_lib, "width": w, "windows": windows,
              "c5_thr_seq": 6.0, "c5_thr_struct": thr_c5}

    sample = sorted(set(int(round(i * (n_lib - 1) / max(1, args.sample_pairs - 1))) for i in range(args.sample_pairs)))
    tj = eff = None
    if not args.plain_only:
        # every pair's T from its own printed sums; the sampled pairs' largest structure score on the way
        k = max(1, int(round(args.total_hits / n_lib)))
        d_S = torch.zeros(1, dtype=torch.float64, device=dev)
        ctx.profile_row_bound_dev(codes_d.data_ptr(), profile_d.data_ptr(), _lib.PROFILE_F32, n_pos, d_S.data_ptr(), None)
        ctx.synchronize()
        S = float(d_S.item())
        tj, eff, share, share_up = np.empty(n_lib), np.empty(n_lib), np.empty(n_lib), np.empty(n_lib)
        st_max = {}
        for i in range(n_lib):
            m0 = ctx.motif(LT[i], LP[i])
            ctx.scan_dev(m0, codes_d.data_ptr(), profile_d.data_ptr(), _lib.PROFILE_F32, n_pos, out_seq.data_ptr(), out_st.data_ptr(), None)
            ctx.synchronize()
            torch.cuda.synchronize()
            m0.close()
            ok = torch.isfinite(out_seq) & torch.isfinite(out_st)
            printed = (torch.round(out_seq * 1000.0) / 1000.0).double() + out_st          # float32 multiply, rint, divide; fp64 add
            printed[~ok] = -float("inf")
            tj[i] = kth_gap(torch, printed, k)
            eff[i] = _lib.library_sum_thresholds(LT[i:i + 1], LP[i:i + 1], -np.inf, tj[i], S)[0]
            f_ok = out_seq[ok].double()
            share[i] = float((f_ok > eff[i]).double().mean())
            slack = _lib.credit_table(LT[i], eff[i], bits=0)[1]
            share_up[i] = float((f_ok > eff[i] - slack).double().mean()) if np.isfinite(slack) else 1.0
            del f_ok
            if i in sample:
                st_max[i] = float(out_st[ok].max())
            del ok, printed

    codes, profile = codes_d.cpu().numpy(), profile_d.cpu().numpy()
    del profile_d, out_st
    torch.cuda.empty_cache()
    ctx.stage(codes, profile)
    lib = ctx.library(LT, LP)
    legs = {}
    small = 1 << 20
    bufs = (np.empty(small, np.int64), np.empty(small, np.int32), np.empty(small, np.float32), np.empty(small, np.float64))

    def plain_c5():
        return len(ctx.library_hits_staged(lib, 6.0, thr_c5)[0])
    legs["plain_c5"] = plain_c5
    if not args.plain_only:
        assert ctx.profile_row_bound_staged() == S
        assert np.array_equal(eff, _lib.library_sum_thresholds(LT, LP, -np.inf, tj, S))
        U = S * np.maximum(LP.max(axis=2), 0.0).sum(axis=1)
        result.update({"row_sum_max": S, "target_hits_per_pair": k, "thr_sum_min_median_max": [float(tj.min()), float(np.median(tj)), float(tj.max())],
                       "thr_eff_min_median_max": [float(eff.min()), float(np.median(eff)), float(eff.max())],
                       "share_of_windows_with_seq_above_thr_eff_min_median_max": [float(share.min()), float(np.median(share)), float(share.max())],
                       "phase_a_survivor_rate": {"lower_bound_mean_over_pairs": float(share.mean()), "upper_bound_mean_over_pairs": float(share_up.mean()),
                                                 "note": "lower: windows with seq > thr_eff; upper: windows with seq > thr_eff - the credit table's slack"},
                       "share_of_windows_with_seq_above_thr_eff": {str(i): float(share[i]) for i in sample},
                       "U_minus_largest_struct_score": {str(i): float(U[i] - st_max[i]) for i in sample},
                       "U": {str(i): float(U[i]) for i in sample}})
        sample_motifs = {i: ctx.motif(LT[i], LP[i]) for i in sample}
        neg = np.full(n_lib, -np.inf)

        def sum_lib():
            return len(ctx.library_hits_sum_staged(lib, -np.inf, -np.inf, tj)[0])

        def per_pair():
            return sum(len(ctx.hits_sum_staged(sample_motifs[i], -np.inf, -np.inf, float(tj[i]))[0]) for i in sample)

        def plain_eff():
            n = ctypes.c_int64(0)
            rc = ctx._L.pfmscan_library_hits_staged(ctx._h, lib._h, eff.ctypes.data, neg.ctypes.data, small, bufs[0].ctypes.data,
                                                    bufs[1].ctypes.data, bufs[2].ctypes.data, bufs[3].ctypes.data, ctypes.byref(n))
            if rc not in (_lib.OK, _lib.E_CAPACITY):
                raise RuntimeError("pfmscan_library_hits_staged: %d" % rc)
            return {"rc": rc, "n_hits_reported": int(n.value)}
        legs.update({"sum": sum_lib, "per_pair_sample": per_pair, "plain_eff": plain_eff})

    counts, times = {}, {name: [] for name in legs}
    for name, f in legs.items():                           # warm: kernels loaded, scratch sized, credit tables built once
        t0 = time.perf_counter()
        counts[name] = f()
        result.setdefault("first_call_ms", {})[name] = round((time.perf_counter() - t0) * 1e3, 2)
    for _ in range(args.blocks):
        for name, f in legs.items():
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result["hits"] = counts
    result["calls_per_leg"] = args.blocks
    result["median_ms"] = {name: round(statistics.median(v), 3) for name, v in times.items()}
    result["all_ms"] = {name: [round(x, 3) for x in v] for name, v in times.items()}
    result["plain_c5_spread_ms"] = round(max(times["plain_c5"]) - min(times["plain_c5"]), 3)
    if not args.plain_only:
        scale = n_lib / float(len(sample))
        result["per_pair_scaled_ms"] = round(result["median_ms"]["per_pair_sample"] * scale, 3)
        result["per_pair_scaling"] = "%d sampled pairs timed, scaled by %g to %d pairs" % (len(sample), scale, n_lib)
        result["sum_over_per_pair_scaled"] = round(result["median_ms"]["sum"] / result["per_pair_scaled_ms"], 4)
        result["sum_over_plain_eff"] = round(result["median_ms"]["sum"] / result["median_ms"]["plain_eff"], 4)
        result["max_prefilter_eps_after_sum"] = None
        sum_lib()
        result["max_prefilter_eps_after_sum"] = lib.info()["max_prefilter_eps"]
        for m0 in sample_motifs.values():
            m0.close()
    lib.close()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
