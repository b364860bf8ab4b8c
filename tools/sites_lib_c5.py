"""Measurements of the library site sums at C5 size (100k records x 3 kb, 256 motifs, w = 12, flank 0): HIP-event
times of whole `pfmscan_site_sums_lib_dev` calls for float32 and float64 rows on random motif-major hit lists of 5e6 and
5e4 hits, beside what the single-motif entry point offers for the same result in the same job -- one
`pfmscan_site_sums_dev` call per motif on that motif's list, the download of the group rows and math.fsum per cell -- and
the host tail of the one-pass route (the accumulators home, normalised and rounded).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel times.

    python tools/sites_lib_c5.py [--records 100000] [--length 3000] [--motifs 256] [--width 12] [--flank 0] [--iters 10]
                                 [--warmup 3] [--hits 5000000,50000] [--fsum-motifs 8] [--loop-iters 3]

math.fsum over every group row of 5e6 hits is minutes of Python: it runs on the first --fsum-motifs motifs and is scaled by
the share of the groups they hold (`fsum_s_scaled`; `fsum_motifs` says how many were summed).  The rounded one-pass sums of
those motifs are compared with it bit for bit (`equal_bits`).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FLOAT_ATOMIC_RATE = 1.3e12   # bytes / s: the chip-wide rate of global FLOAT atomic adds on MI355X, the only measured neighbour


def hit_list(rng, n_motifs, n_rec, L, m, n_hits):
    """about n_hits distinct (motif, window) pairs, motif-major -> (pos int64, motif int32)"""
    nw = L - m + 1
    w = np.unique(rng.integers(0, n_motifs * n_rec * nw, size=n_hits))
    motif, w = w // (n_rec * nw), w % (n_rec * nw)
    return (w // nw) * (L + 1) + w % nw, motif.astype(np.int32)


def timed(call, iters, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--motifs", type=int, default=256)
    ap.add_argument("--width", type=int, default=12)
    ap.add_argument("--flank", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hits", default="5000000,50000")
    ap.add_argument("--fsum-motifs", type=int, default=8)
    ap.add_argument("--loop-iters", type=int, default=3, help="timed repetitions of the one-call-per-motif loop (after one warm-up)")
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib
    n_rec, L, m, F, n_motifs = args.records, args.length, args.width, args.flank, args.motifs
    W = m + 2 * F
    ncell = W * 7
    n_pos = n_rec * (L + 1)
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    offsets = np.arange(n_rec, dtype=np.int64) * (L + 1)
    lengths = np.full(n_rec, L, dtype=np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    off, ln = up(offsets), up(lengths)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    prof32 = torch.rand((n_pos, 7), dtype=torch.float32, device=dev, generator=g)
    prof32.view(n_rec, L + 1, 7)[:, L, :] = 0
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "rows": n_pos, "motifs": n_motifs, "width": m, "flank": F,
           "accumulator_bytes": n_motifs * _lib.SITE_LIMBS * ncell * 8,
           "float_atomic_bytes_per_s": FLOAT_ATOMIC_RATE}
    lists = dict(("hits_%.0e" % int(h), hit_list(rng, n_motifs, n_rec, L, m, int(h))) for h in args.hits.split(","))
    for dtype, name in ((np.float32, "float32"), (np.float64, "float64")):
        prof = prof32 if dtype is np.float32 else prof32.to(torch.float64)
        for label, (pos, mot) in lists.items():
            t0 = time.perf_counter()
            first, rec, gmot = _lib.site_groups_lib(pos, mot, n_motifs, offsets, lengths, m)
            entry = {"hits": int(pos.size), "groups": int(rec.size), "host_groups_s": time.perf_counter() - t0}
            n_grp = rec.size
            d_pos, d_first, d_rec, d_gmot = up(pos), up(first), up(rec), up(gmot)
            acc = torch.empty((n_motifs, _lib.SITE_LIMBS, ncell), dtype=torch.int64, device=dev)

            def one_pass():
                ctx.site_sums_lib_dev(None, prof.data_ptr(), dtype, n_pos, d_pos.data_ptr(), pos.size, d_first.data_ptr(),
                                      d_rec.data_ptr(), d_gmot.data_ptr(), n_grp, off.data_ptr(), ln.data_ptr(), n_rec, n_motifs,
                                      m, F, acc.data_ptr(), None)
            times = timed(one_pass, args.iters, args.warmup)
            med = statistics.median(times)
            # at most three 8-byte adds per non-zero group cell (uniform rows in [0, 1): nearly always three)
            adds = 3 * n_grp * ncell
            entry.update({"lib_call_ms_median": med, "lib_call_ms_min": min(times), "lib_call_ms": times,
                          "atomic_adds_at_most": int(adds), "atomic_bytes_per_s_at_median_at_most": adds * 8 / (med * 1e-3),
                          "fraction_of_float_atomic_rate_at_most": adds * 8 / (med * 1e-3) / FLOAT_ATOMIC_RATE,
                          "row_bytes_read": int(pos.size * ncell * np.dtype(dtype).itemsize)})
            # the host tail: accumulators home, normalised, rounded
            t0 = time.perf_counter()
            raw = acc.cpu().numpy().view(np.uint64)
            t1 = time.perf_counter()
            norm = _lib.site_acc_add(np.zeros_like(raw), raw)
            S = _lib.site_acc_round(norm)
            entry.update({"tail_download_s": t1 - t0, "tail_normalise_round_s": time.perf_counter() - t1})
            # what the single-motif entry point offers: one call per motif, the group rows home, math.fsum
            bounds = np.searchsorted(mot, np.arange(n_motifs + 1))
            per = []
            for k in range(n_motifs):
                p = pos[bounds[k]:bounds[k + 1]]
                f, r = _lib.site_groups(p, offsets, lengths, m)
                per.append((p.size, r.size, up(p), up(f), up(r)))
            sums = torch.empty((max(n_grp, 1), W, 7), dtype=torch.float64, device=dev)
            starts = np.concatenate([[0], np.cumsum([x[1] for x in per])]).astype(np.int64)

            def loop():
                for k, (nh, ng, dp, df, dr) in enumerate(per):
                    if nh:
                        ctx.site_sums_dev(None, prof.data_ptr(), dtype, n_pos, dp.data_ptr(), nh, df.data_ptr(), dr.data_ptr(), ng,
                                          off.data_ptr(), ln.data_ptr(), n_rec, m, F, sums[int(starts[k]):].data_ptr(), None)
            ltimes = timed(loop, args.loop_iters, 1)
            entry.update({"per_motif_loop_ms_median": statistics.median(ltimes), "per_motif_loop_ms": ltimes})
            t0 = time.perf_counter()
            rows = sums.cpu().numpy()
            entry["group_rows_bytes"] = int(rows.nbytes)
            entry["group_rows_download_s"] = time.perf_counter() - t0
            ks = list(range(min(args.fsum_motifs, n_motifs)))
            t0 = time.perf_counter()
            equal = True
            for k in ks:
                cols = np.ascontiguousarray(rows[int(starts[k]):int(starts[k + 1])].reshape(-1, ncell).T)
                total = np.asarray([math.fsum(cols[e].tolist()) for e in range(ncell)])
                equal = equal and bool(np.array_equal(total.view(np.uint64), S[k].view(np.uint64)))
            dt = time.perf_counter() - t0
            share = float(starts[len(ks)]) / max(float(starts[-1]), 1.0)
            entry.update({"fsum_motifs": len(ks), "fsum_s_measured": dt, "fsum_s_scaled": dt / share if share else 0.0, "equal_bits": equal})
            entry["per_motif_route_s"] = entry["per_motif_loop_ms_median"] * 1e-3 + entry["group_rows_download_s"] + entry["fsum_s_scaled"]
            entry["one_pass_route_s"] = med * 1e-3 + entry["tail_download_s"] + entry["tail_normalise_round_s"]
            res["%s_%s" % (name, label)] = entry
            del sums, rows, per
        del prof
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
