"""Measurements of the letter-pair counts under hits (`pfmscan_site_joint_dev`) at C3 size (100k records x 3 kb,
w = 12, flank 0, both code streams made on the device): HIP-event times of whole calls -- the memset of the table, the
kernel, the verdict and its one synchronise -- on random hit lists, each beside its neighbours IN THE SAME JOB, alternating:

  single motif, 3e4 and 3e6 hits:  `pfmscan_site_joint_dev` on both streams and on the sequence codes alone, against the
                                   counts-only `pfmscan_site_sums_dev` call on the sequence codes with the same hits (one
                                   stream, no pair table), and against numpy counting both streams on one host thread;
  256 motifs, 5e6 hits:            `pfmscan_site_joint_dev`, against the counts-only `pfmscan_site_sums_lib_dev` call (the
                                   same-row global atomics of k_site_sums_lib) on the same list;
  the slice sweep:                 the same calls with PFMSCAN_SITE_JOINT_SLICE set, i.e. more or fewer flushes of the LDS
                                   table per hit.

The device tables are compared with the numpy count (and with each other's marginals) at the sizes timed.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel times.

    python tools/site_joint_ab.py [--records 100000] [--length 3000] [--width 12] [--flank 0] [--motifs 256] [--iters 20]
                                  [--warmup 3] [--hits 30000,3000000] [--lib-hits 5000000] [--slices 256,4096,65536]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hit_list(rng, n_motifs, n_rec, L, m, n_hits):
    """about n_hits distinct (motif, window) pairs, motif-major -> (pos int64, motif int32)"""
    nw = L - m + 1
    w = np.unique(rng.integers(0, n_motifs * n_rec * nw, size=n_hits))
    motif, w = w // (n_rec * nw), w % (n_rec * nw)
    return (w // nw) * (L + 1) + w % nw, motif.astype(np.int32)


def numpy_joint(codes, codes2, pos, m, flank):
    """the single-motif table on one host thread: a gather and a bincount per column (every column inside its record here)"""
    W = m + 2 * flank
    out = np.zeros((W, 64), dtype=np.int64)
    for j in range(W):
        x = pos - flank + j
        out[j] = np.bincount((codes[x] & 7).astype(np.int64) * 8 + (codes2[x] & 7), minlength=64)
    return out.reshape(1, W, 8, 8)


def timed_alternating(calls, iters, warmup):
    """{name: [ms]}: the calls take turns inside every repetition, each between two HIP events that end in a synchronise"""
    import torch
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = dict((name, []) for name in calls)
    for _ in range(iters):
        for name, call in calls.items():
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--width", type=int, default=12)
    ap.add_argument("--flank", type=int, default=0)
    ap.add_argument("--motifs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hits", default="30000,3000000")
    ap.add_argument("--lib-hits", type=int, default=5000000)
    ap.add_argument("--slices", default="256,4096,65536")
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib
    n_rec, L, m, F, n_motifs = args.records, args.length, args.width, args.flank, args.motifs
    W = m + 2 * F
    n_pos = n_rec * (L + 1)
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    offsets = np.arange(n_rec, dtype=np.int64) * (L + 1)
    lengths = np.full(n_rec, L, dtype=np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    off, ln = up(offsets), up(lengths)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    codes = torch.randint(0, 4, (n_pos,), dtype=torch.uint8, device=dev, generator=g)
    codes2 = torch.randint(0, 7, (n_pos,), dtype=torch.uint8, device=dev, generator=g)
    codes.view(n_rec, L + 1)[:, L] = 7
    codes2.view(n_rec, L + 1)[:, L] = 7
    h_codes, h_codes2 = codes.cpu().numpy(), codes2.cpu().numpy()
    rng = np.random.default_rng(2)
    res = {"records": n_rec, "length": L, "positions": n_pos, "width": m, "flank": F, "motifs": n_motifs,
           "site_joint_cols": _lib.SITE_JOINT_COLS, "device": ctx.device_info()}

    def joint_call(d_pos, d_mot, n_hits, k, table, second=True):
        def call():
            ctx.site_joint_dev(codes, codes2 if second else None, n_pos, d_pos, d_mot, n_hits, off, ln, n_rec, k, m, F, table)
        return call

    def with_slice(call, value):
        def wrapped():
            os.environ["PFMSCAN_SITE_JOINT_SLICE"] = value
            try:
                call()
            finally:
                del os.environ["PFMSCAN_SITE_JOINT_SLICE"]
        return wrapped

    # ---- one motif
    for h in args.hits.split(","):
        pos, _ = hit_list(rng, 1, n_rec, L, m, int(h))
        first, rec = _lib.site_groups(pos, offsets, lengths, m)
        d_pos, d_first, d_rec = up(pos), up(first), up(rec)
        joint = torch.empty((1, W, 8, 8), dtype=torch.int64, device=dev)
        joint1 = torch.empty((1, W, 8, 8), dtype=torch.int64, device=dev)
        counts = torch.empty((max(rec.size, 1), W, 8), dtype=torch.int32, device=dev)

        def counts_only():
            ctx.site_sums_dev(codes, None, np.float32, n_pos, d_pos, pos.size, d_first, d_rec, rec.size, off, ln, n_rec, m, F, None, counts)
        calls = {"site_joint_dev_both_streams": joint_call(d_pos, None, pos.size, 1, joint),
                 "site_joint_dev_codes_only": joint_call(d_pos, None, pos.size, 1, joint1, second=False),
                 "site_sums_dev_counts_only": counts_only}
        for s in args.slices.split(","):
            calls["site_joint_dev_both_streams_slice_%s" % s] = with_slice(joint_call(d_pos, None, pos.size, 1, joint), s)
        times = timed_alternating(calls, args.iters, args.warmup)
        entry = {"hits": int(pos.size), "groups": int(rec.size)}
        entry.update(dict((name, spread(ms)) for name, ms in times.items()))
        calls["site_joint_dev_both_streams"]()
        ctx.synchronize()
        got, got1 = joint.cpu().numpy(), joint1.cpu().numpy()
        t0 = time.perf_counter()
        want = numpy_joint(h_codes, h_codes2, pos, m, F)
        entry["numpy_one_thread_s"] = time.perf_counter() - t0
        entry["equal_to_numpy"] = bool(np.array_equal(got, want))
        entry["codes_only_equals_the_marginal"] = bool(np.array_equal(got1[..., 0], want.sum(axis=3)))
        entry["site_sums_counts_equal_the_marginal"] = bool(np.array_equal(counts.cpu().numpy().astype(np.int64).sum(axis=0), want[0].sum(axis=2)))
        # what the kernel moves: two bytes per hit and column gathered, 8 + 8 (+ 4) bytes per hit of the list and record table reads
        entry["bytes_gathered"] = int(pos.size) * W * 2
        res["one_motif_hits_%.0e" % int(h)] = entry

    # ---- a library
    pos, mot = hit_list(rng, n_motifs, n_rec, L, m, args.lib_hits)
    first, rec, gmot = _lib.site_groups_lib(pos, mot, n_motifs, offsets, lengths, m)
    d_pos, d_mot, d_first, d_rec, d_gmot = up(pos), up(mot), up(first), up(rec), up(gmot)
    joint = torch.empty((n_motifs, W, 8, 8), dtype=torch.int64, device=dev)
    counts = torch.empty((n_motifs, W, 8), dtype=torch.int64, device=dev)

    def lib_counts_only():
        ctx.site_sums_lib_dev(codes, None, np.float32, n_pos, d_pos, pos.size, d_first, d_rec, d_gmot, rec.size, off, ln, n_rec,
                              n_motifs, m, F, None, counts)
    calls = {"site_joint_dev_both_streams": joint_call(d_pos, d_mot, pos.size, n_motifs, joint),
             "site_sums_lib_dev_counts_only": lib_counts_only}
    for s in args.slices.split(","):
        calls["site_joint_dev_both_streams_slice_%s" % s] = with_slice(joint_call(d_pos, d_mot, pos.size, n_motifs, joint), s)
    times = timed_alternating(calls, args.iters, args.warmup)
    entry = {"hits": int(pos.size), "groups": int(rec.size)}
    entry.update(dict((name, spread(ms)) for name, ms in times.items()))
    calls["site_joint_dev_both_streams"]()
    ctx.synchronize()
    got = joint.cpu().numpy()
    bounds = np.searchsorted(mot, np.arange(n_motifs + 1))
    ks = [0, n_motifs // 2, n_motifs - 1]
    entry["equal_to_numpy_motifs"] = ks
    entry["equal_to_numpy"] = bool(all(np.array_equal(got[k:k + 1], numpy_joint(h_codes, h_codes2, pos[bounds[k]:bounds[k + 1]], m, F)) for k in ks))
    entry["site_sums_lib_counts_equal_the_marginal"] = bool(np.array_equal(counts.cpu().numpy(), got.sum(axis=3)))
    res["library_hits_%.0e" % args.lib_hits] = entry
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
