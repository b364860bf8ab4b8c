#!/usr/bin/env python3
"""Fragment averaging, measured (profiles/average/).

  python tools/average_e2e.py kernel [--records 100000 --length 3000]
      C3 scale on the device alone: fragment letters made on the device from a few template structures (w = 100,
      o = 95: 6.0 x 10^7 fragments, 6.0 x 10^9 letters), annotated (pfmscan_dotbracket_annotate_dev) and averaged
      (pfmscan_average_dev) into float64 rows.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel times;
      it prints the wall time of each step and the algorithmic bytes of the averaging (letters read once + rows written).
  python tools/average_e2e.py build [--records 10000 --length 3000] --out DIR
      writes a fragment FASTA of that size, runs `build --format store` on it with the per-stage wall breakdown
      (read / index, T, device, store write), and a numpy CPU restatement of the averaging on the same input.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

W, O = 100, 95


K = 4                       # template structures per fragment length


def templates(rng):
    """tm[n][k]: K balanced random structures of every length n = 1 .. W (fragment f of length n takes tm[n][f % K])"""
    from dotbracket_rules import random_structure
    tm = [[""] * K]
    for n in range(1, W + 1):
        row = []
        while len(row) < K:
            s = random_structure(rng, n)
            if "." in s or n < 3:
                row.append(s)
        tm.append(row)
    return tm


def kernel(args):
    import torch
    from rnascan_amd import _lib, average, dotbracket
    rng = np.random.default_rng(1)
    R, L = args.records, args.length
    rec, start = average.window_starts(np.full(R, L), W, O)
    pos = np.maximum(start, 0)
    flen = np.minimum(start + W, L) - pos
    F = rec.size
    frag_off = np.zeros(F, dtype=np.int64)
    frag_off[1:] = np.cumsum(flen + 1)[:-1]
    n_letters = int((flen + 1).sum())
    rec_row = np.arange(R, dtype=np.int64) * (L + 1)
    frag_row = rec_row[rec] + pos
    rec_frag = np.append(np.searchsorted(rec, np.arange(R)), F).astype(np.int64)
    dev = torch.device("cuda:0")
    # letters: fragment f of length n takes template tm[n][f % K]
    tm = templates(rng)
    pad = np.zeros((W + 1, K, W), dtype=np.uint8)
    for n in range(1, W + 1):
        for k in range(K):
            pad[n, k, :n] = dotbracket.LUT[np.frombuffer(tm[n][k].encode(), dtype=np.uint8)]
    tmpl = torch.from_numpy(pad).to(dev)
    d_codes = torch.full((n_letters,), 7, dtype=torch.uint8, device=dev)
    chunk = 1 << 22
    for a in range(0, F, chunk):
        b = min(F, a + chunk)
        fl = torch.from_numpy(flen[a:b]).to(dev)
        fo = torch.from_numpy(frag_off[a:b]).to(dev)
        n = int(flen[a:b].sum())
        idx = torch.repeat_interleave(torch.arange(b - a, device=dev), fl)
        within = torch.arange(n, device=dev) - torch.repeat_interleave(torch.cumsum(fl, 0) - fl, fl)
        t = (torch.arange(a, b, device=dev) % K)[idx]
        d_codes[fo[idx] + within] = tmpl[fl[idx], t, within]
    torch.cuda.synchronize()
    d_letters = torch.empty_like(d_codes)
    tabs = [torch.from_numpy(x).to(dev) for x in (frag_off, flen, frag_row, rec_row, np.full(R, L, np.int64), rec_frag)]
    n_max = 20
    T = torch.from_numpy(average.value_table(n_max).copy()).to(dev)
    n_rows = R * (L + 1)
    out = torch.empty((n_rows, 7), dtype=torch.float64, device=dev)
    res = {"records": R, "length": L, "fragments": F, "letters": int(flen.sum()), "rows": n_rows}
    with _lib.Context(0) as ctx:
        for rep in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.dotbracket_annotate_dev(d_codes, d_letters, n_letters, letter_map=[1, 2, 6, 0, 3, 5, 4])
            ctx.synchronize()
            t1 = time.perf_counter()
            ctx.average_dev(d_letters, n_letters, tabs[0], tabs[1], tabs[2], F, W, tabs[3], tabs[4], tabs[5], R, n_rows, T,
                            n_max, out)
            ctx.synchronize()
            t2 = time.perf_counter()
            res.setdefault("annotate_wall_s", []).append(round(t1 - t0, 5))
            res.setdefault("average_wall_s", []).append(round(t2 - t1, 5))
    res["average_bytes"] = int(flen.sum()) + n_rows * 56
    # spot check: a sample of rows against the host restatement of its record
    from average_rules import counts
    from dotbracket_rules import annotate
    for r in (0, R // 2, R - 1):
        sel = np.flatnonzero(rec == r)
        c = counts(pos[sel].tolist(), [annotate(tm[int(flen[f])][f % K]) for f in sel.tolist()], L)
        want = average.value_table(n_max)[c.sum(1)[:, None] * (c.sum(1)[:, None] + 1) // 2 + c]
        got = out[r * (L + 1):r * (L + 1) + L].cpu().numpy()
        assert np.array_equal(got, want), "record %d differs" % r
    res["spot_check"] = "3 records equal the host restatement"
    print(json.dumps(res))


def build(args):
    from dotbracket_rules import annotate
    from rnascan_amd import _lib, average
    rng = np.random.default_rng(2)
    os.makedirs(args.out, exist_ok=True)
    fa = os.path.join(args.out, "frags.fa")
    tm = templates(rng)
    R, L = args.records, args.length
    rec, start = average.window_starts(np.full(R, L), W, O)
    pos = np.maximum(start, 0)
    flen = np.minimum(start + W, L) - pos
    t = time.perf_counter()
    with open(fa, "w") as f:
        for k in range(rec.size):
            f.write(">r%06d_frag_%d\n%s\n" % (rec[k], start[k], tm[flen[k]][k % K]))
    res = {"records": R, "length": L, "fragments": int(rec.size), "write_input_s": round(time.perf_counter() - t, 3)}
    stats = {}
    with _lib.Context(0) as ctx:
        average.build(ctx, fa, os.path.join(args.out, "store_warm"), stats={})
        t = time.perf_counter()
        average.build(ctx, fa, os.path.join(args.out, "store"), stats=stats)
        res["build_wall_s"] = round(time.perf_counter() - t, 3)
    res["stages_s"] = {k: round(v, 3) for k, v in stats.items()}
    # numpy CPU baseline on the same fragments: align, count, normalise (letters annotated once per template, untimed)
    col = np.full(256, 7, dtype=np.int64)
    for i, ch in enumerate("BEHLMRT"):
        col[ord(ch)] = i
    ann_codes = [[col[np.frombuffer(annotate(x).encode(), dtype=np.uint8)] for x in row] for row in tm]
    first = np.append(np.searchsorted(rec, np.arange(R)), rec.size)
    t = time.perf_counter()
    for r in range(R):
        c = np.zeros((L, 7), dtype=np.int64)
        for f in range(int(first[r]), int(first[r + 1])):
            n = int(flen[f])
            c[np.arange(pos[f], pos[f] + n), ann_codes[n][f % K]] += 1
        _ = c / c.sum(1, keepdims=True)
    res["numpy_cpu_s"] = round(time.perf_counter() - t, 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--records", type=int, default=100000)
    k.add_argument("--length", type=int, default=3000)
    k.add_argument("--reps", type=int, default=3)
    b = sub.add_parser("build")
    b.add_argument("--records", type=int, default=10000)
    b.add_argument("--length", type=int, default=3000)
    b.add_argument("--out", required=True)
    args = ap.parse_args()
    kernel(args) if args.cmd == "kernel" else build(args)


if __name__ == "__main__":
    main()
