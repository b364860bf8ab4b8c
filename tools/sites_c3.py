"""Measurements of the site sums at C3 size (100k records x 3 kb, w = 12): run under `rocprofv3 --kernel-trace --stats` for
the kernel times; prints HIP-event times of whole `pfmscan_site_sums_dev` calls for float32 and float64 rows at
two hit rates, wall times of `pfmscan_site_sums_staged` over the same staged float32 stream, the algorithmic bytes over the
time as a fraction of the HBM peak, the numpy time of the same sums on a sample of the hits, and the math.fsum time over the
group rows.

    python tools/sites_c3.py [--records 100000] [--length 3000] [--width 12] [--flank 0] [--iters 10] [--warmup 3] [--no-staged]
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
HBM_PEAK = 8.0e12            # bytes / s, MI355X


def hit_list(rng, n_rec, L, m, rate):
    """about rate x (all windows) distinct window starts, sorted, as stream positions"""
    nw = L - m + 1
    w = np.unique(rng.integers(0, n_rec * nw, size=int(rate * n_rec * nw)))
    return (w // nw) * (L + 1) + w % nw


def numpy_sums(rows, pos, W, flank, L):
    """the same sums on the host for hits ``pos`` (flanks clipped at the record ends), plain numpy -> (seconds, [W][7])"""
    t0 = time.perf_counter()
    x = pos[:, None] - flank + np.arange(W)
    start = pos % (L + 1)
    ok = (start[:, None] - flank + np.arange(W) >= 0) & (start[:, None] - flank + np.arange(W) < L)
    out = np.where(ok[..., None], rows[np.where(ok, x, 0)].astype(np.float64), 0.0).sum(axis=0)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--width", type=int, default=12)
    ap.add_argument("--flank", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-staged", action="store_true", help="skip the staged form (it needs the float32 rows on the host)")
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib
    n_rec, L, m, F = args.records, args.length, args.width, args.flank
    W = m + 2 * F
    n_pos = n_rec * (L + 1)
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    offsets = np.arange(n_rec, dtype=np.int64) * (L + 1)
    lengths = np.full(n_rec, L, dtype=np.int64)
    off, ln = torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    prof32 = torch.rand((n_pos, 7), dtype=torch.float32, device=dev, generator=g)
    prof32.view(n_rec, L + 1, 7)[:, L, :] = 0
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "rows": n_pos, "width": m, "flank": F, "hbm_peak_bytes_per_s": HBM_PEAK}
    lists = {"rate_1e-4": hit_list(rng, n_rec, L, m, 1e-4), "rate_1e-2": hit_list(rng, n_rec, L, m, 1e-2)}
    host_rows = None
    for dtype, name in ((np.float32, "float32"), (np.float64, "float64")):
        prof = prof32 if dtype is np.float32 else prof32.to(torch.float64)
        for label, pos in lists.items():
            first, rec = _lib.site_groups(pos, offsets, lengths, m)
            n_grp = rec.size
            d_pos, d_first, d_rec = (torch.from_numpy(a).to(dev) for a in (pos, first, rec))
            sums = torch.empty((n_grp, W, 7), dtype=torch.float64, device=dev)

            def call():
                ctx.site_sums_dev(None, prof.data_ptr(), dtype, n_pos, d_pos.data_ptr(), pos.size, d_first.data_ptr(), d_rec.data_ptr(),
                                  n_grp, off.data_ptr(), ln.data_ptr(), n_rec, m, F, sums.data_ptr(), None)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            times = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(args.iters):
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            med = statistics.median(times)
            nbytes = pos.size * W * 7 * np.dtype(dtype).itemsize + 8 * pos.size + n_grp * W * 7 * 8
            entry = {"hits": int(pos.size), "groups": int(n_grp), "call_ms_median": med, "call_ms_min": min(times), "call_ms": times,
                     "algorithmic_bytes": int(nbytes), "fraction_of_hbm_peak_at_median": nbytes / (med * 1e-3) / HBM_PEAK}
            if dtype is np.float32:
                # the host: plain numpy over a sample of the hits, and math.fsum over every group row
                if host_rows is None:
                    host_rows = prof32.cpu().numpy()
                sample = pos[:min(pos.size, 200000)]
                dt, _ = numpy_sums(host_rows, sample, W, F, L)
                entry["numpy_s_for_all_hits_one_thread"] = dt * pos.size / sample.size
                rows = sums.cpu().numpy().reshape(n_grp, W * 7)
                t0 = time.perf_counter()
                cols = np.ascontiguousarray(rows.T)
                total = [math.fsum(cols[e].tolist()) for e in range(W * 7)]
                entry["fsum_s"] = time.perf_counter() - t0
                _, want = numpy_sums(host_rows, pos, W, F, L) if pos.size <= 400000 else (0, None)
                if want is not None:
                    entry["max_rel_diff_vs_numpy"] = float(np.abs(np.asarray(total).reshape(W, 7) - want).max() / want.max())
            res["%s_%s" % (name, label)] = entry
        del prof
    if not args.no_staged:
        ctx.stage(None, host_rows)
        for label, pos in lists.items():
            for _ in range(args.warmup):
                ctx.site_sums_staged(pos, offsets, lengths, m, F, letters=False)
            times = []
            for _ in range(args.iters):
                t0 = time.perf_counter()
                ctx.site_sums_staged(pos, offsets, lengths, m, F, letters=False)
                times.append((time.perf_counter() - t0) * 1e3)
            res["float32_%s" % label]["staged_wall_ms_median"] = statistics.median(times)
            res["float32_%s" % label]["staged_wall_ms"] = times
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
