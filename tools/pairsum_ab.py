"""Cost of the joint threshold of the two-FASTA mode (pfmscan_hits_pair_sum_dev) at C3 size, one process.

    python tools/pairsum_ab.py [--records 100000] [--length 3000] [--width 12] [--hit-rate 1e-4] [--cli-records 1000]

Two synthetic code streams (4 sequence letters, 7 structure letters, a separator after every record) are made on the
device.  T is the printed sum between the k-th and (k+1)-th largest, k = hit rate x windows.  Medians of 10 calls after 3
warm-ups, HIP events on the stream the call runs on (hit counter zeroed outside the timed span):
  1. sum_inf     hits_pair_sum_dev(thr = -inf, T)                   k_pair_cred_sum (the route taken is in the output)
     dense_inf   the same call with PFMSCAN_CREDITS=0 in a second ctx  k_pair_sum_dense
     host_filter the route the scanner took before: both all-scores passes, both arrays home, the filter in numpy (wall clock)
     plain_m6    hits_pair_dev(thr = 6)                             k_letters_cred<.., PAIR>
  2. sum_m6      hits_pair_sum_dev(thr = 6, T6) against plain_m6    k_letters_cred<.., PAIR, SUM>; T6 = the median printed sum
                 of plain_m6's hits
  4. the whole command `rnascan -m ' -inf' --min-seqstruct T` on --cli-records records, with the device call and with the
     finished-rows filter (the same engine without hits_pair_sum), wall clock.
  3. library_ms  library_hits_letters_sum_dev, --library-pairs pairs in one pass, against as many single calls (16 sampled, scaled).
One JSON line."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def kth_gap(torch, x, k):
    top = torch.topk(x, k + 1).values
    return 0.5 * (float(top[k - 1]) + float(top[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--width", type=int, default=12)
    ap.add_argument("--hit-rate", type=float, default=1e-4)
    ap.add_argument("--host-filter-reps", type=int, default=2)
    ap.add_argument("--cli-records", type=int, default=1000)
    ap.add_argument("--library-pairs", type=int, default=256)
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib, pack
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    w = args.width
    n_pos = args.records * (args.length + 1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241019)
    sep = (torch.arange(n_pos, device=dev) % (args.length + 1)) == args.length
    codes = torch.randint(0, 4, (n_pos,), dtype=torch.uint8, device=dev, generator=gen)
    codes2 = torch.randint(0, 7, (n_pos,), dtype=torch.uint8, device=dev, generator=gen)
    codes[sep] = pack.SEP
    codes2[sep] = pack.SEP
    del sep
    rng = np.random.default_rng(5)
    T1 = np.full((w, 8), np.nan)
    T1[:, :4] = np.log2(rng.dirichlet(np.full(4, 0.5), size=w) * 4.0 + 0.01)
    T2 = np.full((w, 8), np.nan)
    T2[:, :7] = np.log2(rng.dirichlet(np.full(7, 0.5), size=w) * 7.0 + 0.01)
    a, b = ctx.motif(T1, None), ctx.motif(T2, None)
    windows = args.records * (args.length - w + 1)
    k = max(1, int(round(args.hit_rate * windows)))

    out_seq = torch.zeros(n_pos, dtype=torch.float32, device=dev)
    out_st = torch.zeros(n_pos, dtype=torch.float64, device=dev)
    ctx.scan_dev(a, codes.data_ptr(), None, _lib.PROFILE_NONE, n_pos, out_seq.data_ptr(), None, None)
    ctx.scan_letters_f64_dev(b, codes2.data_ptr(), n_pos, out_st.data_ptr(), None)
    ctx.synchronize()
    printed = (torch.round(out_seq * 1000.0) / 1000.0).double() + torch.round(out_st * 1000.0) / 1000.0
    printed = torch.where(torch.isfinite(printed), printed, torch.full_like(printed, -float("inf")))
    thr_sum = kth_gap(torch, printed, k)
    m6 = torch.isfinite(printed) & (out_seq > 6.0) & (out_st > 6.0)
    n_m6 = int(m6.sum())
    thr_sum6 = float(torch.median(printed[m6])) if n_m6 else 0.0
    del printed, m6, out_seq, out_st

    cap = max(4 * k, 2 * n_m6, 1 << 16)
    hp = torch.empty(cap, dtype=torch.int64, device=dev)
    hq = torch.empty(cap, dtype=torch.float32, device=dev)
    ht = torch.empty(cap, dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)

    def timed(call):
        ms, n = [], 0
        for it in range(13):
            cnt.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record(side)
                call()
                e1.record(side)
            side.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
            n = int(cnt.item())
        return round(statistics.median(ms), 4), round(min(ms), 4), n

    ptrs = (cap, hp.data_ptr(), hq.data_ptr(), ht.data_ptr(), cnt.data_ptr())
    res = {"records": args.records, "length": args.length, "width": w, "windows": windows, "target_hits": k, "thr_sum": thr_sum, "thr_sum_m6": thr_sum6}
    res["sum_inf_ms"] = timed(lambda: ctx.hits_pair_sum_dev(a, b, codes.data_ptr(), codes2.data_ptr(), n_pos, -np.inf, -np.inf, thr_sum, *ptrs, stream=side.cuda_stream))
    res["sum_inf_route"] = ctx.pair_sum_route()
    os.environ["PFMSCAN_CREDITS"] = "0"                 # read when a ctx is made: no integer prefilter -> the exact kernel
    ctx0 = _lib.Context(0)
    a0, b0 = ctx0.motif(T1, None), ctx0.motif(T2, None)
    del os.environ["PFMSCAN_CREDITS"]
    res["dense_inf_ms"] = timed(lambda: ctx0.hits_pair_sum_dev(a0, b0, codes.data_ptr(), codes2.data_ptr(), n_pos, -np.inf, -np.inf, thr_sum, *ptrs, stream=side.cuda_stream))
    res["dense_inf_route"] = ctx0.pair_sum_route()
    a0.close()
    b0.close()
    ctx0.close()
    res["plain_m6_ms"] = timed(lambda: ctx.hits_pair_dev(a, b, codes.data_ptr(), codes2.data_ptr(), n_pos, 6.0, 6.0, *ptrs, stream=side.cuda_stream))
    res["sum_m6_ms"] = timed(lambda: ctx.hits_pair_sum_dev(a, b, codes.data_ptr(), codes2.data_ptr(), n_pos, 6.0, 6.0, thr_sum6, *ptrs, stream=side.cuda_stream))
    res["sum_m6_route"] = ctx.pair_sum_route()

    # 3. a library of pairs in ONE pass (k_library<.., uint8_t, true, SUM>) against one hits_pair_sum_dev call per pair: tables drawn like
    # pair 0's, the same T for every pair, thr = -inf; 3 library calls after one warm-up, 16 single calls sampled and scaled
    if args.library_pairs > 0:
        n = args.library_pairs
        LT = np.full((n, w, 8), np.nan)
        LS = np.full((n, w, 8), np.nan)
        LT[:, :, :4] = np.log2(rng.dirichlet(np.full(4, 0.5), size=(n, w)) * 4.0 + 0.01)
        LS[:, :, :7] = np.log2(rng.dirichlet(np.full(7, 0.5), size=(n, w)) * 7.0 + 0.01)
        eff = _lib.library_letters_sum_thresholds(LT, LS, -np.inf, thr_sum)
        res["library_pairs"] = n
        res["library_thr_eff"] = [round(float(eff.min()), 3), round(float(np.median(eff)), 3), round(float(eff.max()), 3)]
        lcap = 1 << 24
        lp = torch.empty(lcap, dtype=torch.int64, device=dev)
        lm = torch.empty(lcap, dtype=torch.int32, device=dev)
        lq = torch.empty(lcap, dtype=torch.float32, device=dev)
        lt = torch.empty(lcap, dtype=torch.float64, device=dev)
        lib = ctx.library(LT, struct_letters=LS)
        ms = []
        for it in range(4):
            cnt.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record(side)
                ctx.library_hits_letters_sum_dev(lib, codes.data_ptr(), codes2.data_ptr(), n_pos, -np.inf, -np.inf, thr_sum, lcap, lp.data_ptr(),
                                                 lm.data_ptr(), lq.data_ptr(), lt.data_ptr(), cnt.data_ptr(), stream=side.cuda_stream)
                e1.record(side)
            side.synchronize()
            if it >= 1:
                ms.append(e0.elapsed_time(e1))
        res["library_ms"] = [round(statistics.median(ms), 3), round(min(ms), 3), int(cnt.item())]
        lib.close()
        single, hits = [], 0
        for k in range(min(16, n)):
            ak, bk = ctx.motif(LT[k], None), ctx.motif(LS[k], None)
            med, _, nh = timed(lambda: ctx.hits_pair_sum_dev(ak, bk, codes.data_ptr(), codes2.data_ptr(), n_pos, -np.inf, -np.inf, thr_sum, *ptrs, stream=side.cuda_stream))
            single.append(med)
            hits += nh
            ak.close()
            bk.close()
        res["single_calls_sampled"] = len(single)
        res["single_calls_ms_scaled"] = round(sum(single) / len(single) * n, 3)
        res["single_calls_hits_sampled"] = hits
        del lp, lm, lq, lt

    # the route before: both all-scores passes, both arrays home, the filter on the host
    h1, h2 = codes.cpu().numpy(), codes2.cpu().numpy()
    host = []
    n_host = -1
    for _ in range(args.host_filter_reps):
        t0 = time.perf_counter()
        ctx.stage(h1, None)
        sq, _ = ctx.scan_staged(a)
        st = ctx.scan_letters_f64_host(b, h2)
        with np.errstate(invalid="ignore"):
            pos = np.flatnonzero(np.isfinite(sq) & np.isfinite(st))
            pos = pos[np.round(sq[pos], 3).astype(np.float64) + _lib.round_decimals(st[pos], 3) > thr_sum]
        host.append(round((time.perf_counter() - t0) * 1e3, 1))
        n_host = int(pos.size)
        del sq, st, pos
    res["host_filter_ms"] = host
    res["host_filter_hits"] = n_host
    a.close()
    b.close()
    ctx.close()

    if args.cli_records > 0:
        from rnascan_amd import cli, scanner

        class RowsFilterEngine(scanner.HipEngine):
            def __getattribute__(self, name):
                if name == "hits_pair_sum":
                    raise AttributeError(name)
                return object.__getattribute__(self, name)

        tmp = tempfile.mkdtemp(prefix="pairsum_ab_")
        with open(os.path.join(tmp, "sq.pfm"), "w") as f, open(os.path.join(tmp, "st.pfm"), "w") as g:
            f.write("PO\tA\tC\tG\tU\n")
            g.write("PO\t" + "\t".join("EHTBLRM") + "\n")
            for j in range(w):
                f.write(str(j) + "\t" + "\t".join("%.5f" % x for x in rng.dirichlet(np.full(4, 0.5))) + "\n")
                g.write(str(j) + "\t" + "\t".join("%.5f" % x for x in rng.dirichlet(np.full(7, 0.5))) + "\n")
        with open(os.path.join(tmp, "s.fa"), "w") as f, open(os.path.join(tmp, "t.fa"), "w") as g:
            for i in range(args.cli_records):
                f.write(">r%d\n%s\n" % (i, "".join(rng.choice(list("ACGU"), size=args.length))))
                g.write(">r%d\n%s\n" % (i, "".join(rng.choice(list("EHTBLRM"), size=args.length))))
        argv = ["-p", os.path.join(tmp, "sq.pfm"), "-q", os.path.join(tmp, "st.pfm"), "-u", "-m", " -inf", "--min-seqstruct", "9.0",
                os.path.join(tmp, "s.fa"), os.path.join(tmp, "t.fa")]
        cli_ms = {}
        for name, cls in (("device", scanner.HipEngine), ("rows_filter", RowsFilterEngine)):
            eng = cls(0)
            t = []
            for _ in range(2):
                out = io.StringIO()
                t0 = time.perf_counter()
                cli.main(argv, engine=eng, out=out)
                t.append(round((time.perf_counter() - t0) * 1e3, 1))
            cli_ms[name] = t
            cli_ms[name + "_rows"] = out.getvalue().count("\n") - 1
            eng.close()
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
        res["cli_records"] = args.cli_records
        res["cli_ms"] = cli_ms
    print(json.dumps(res))


if __name__ == "__main__":
    main()
