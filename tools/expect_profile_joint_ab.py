"""Measurements of the expected nucleotide x context table on averaged-structure profiles (DESIGN 5i,
`pfmscan_expect_profile_joint_dev`) at C3 size (100k records x 3 kb, float32 rows and codes made on the device), the routes
taking turns inside every repetition IN THE SAME JOB:

  route EP  `pfmscan_expect_profile_dev` in joint form with both margins: the part of the call that existed before -- the
            yardstick;
  route JM  `pfmscan_expect_profile_joint_dev`, the table and both margins;
  route J   `pfmscan_expect_profile_joint_dev`, the table alone (both margins NULL);
  route EP0 route EP through ANOTHER build of the library (`--baseline-lib`, the commit before the table: loaded beside this
            one, its own context on the same device, the same buffers), to hold the calls without the table to that build's
            run-to-run spread;
  route EP1 route EP of THIS build called the way route EP0 is (a second context of its own, the same raw call): what EP0 is
            compared with, so that the context and the call path are not part of the difference;

all in PFMSCAN_EXPECT_POSTERIOR mode with the occupancy and Windows, one motif pair per width and a library (`--cases`), each 5
times after 2 warm-ups: medians and the spread (min, max).  A call is timed by the host clock from before the enqueue to the
return of `pfmscan_synchronize`.  At the size timed the margins of route JM are compared with route EP's by the wrapping sums of
their bit patterns, and the table's sum over the nucleotides with exp_struct to a printed difference.  Run it under
`rocprofv3 --kernel-trace --stats` for the level-0 kernel's share, and under `--pmc` in a run of its own for counters.
The table takes 32 m doubles per record and motif: `--records` of a library case bounds it (`width:motifs:records`).

    python tools/expect_profile_joint_ab.py [--records 100000] [--length 3000] [--cases 8:1,12:1,18:1,12:256:4096] [--iters 5] [--warmup 2]
                                            [--baseline-lib FILE] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occupancy_profile_ab import seq_table, spread, struct_tables, timed_alternating  # noqa: E402  (tools/ is the script's own directory)


class Baseline(object):
    """`pfmscan_expect_profile_dev` of another build of the library, on a context of its own"""

    def __init__(self, path):
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        self.L = L = ctypes.CDLL(path)
        L.pfmscan_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
        L.pfmscan_ctx_destroy.argtypes = [vp]
        L.pfmscan_ctx_destroy.restype = None
        L.pfmscan_synchronize.argtypes = [vp]
        L.pfmscan_expect_profile_dev.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp]
        self.h = vp()
        if L.pfmscan_ctx_create(0, ctypes.byref(self.h)) != 0:
            raise RuntimeError("the baseline library made no context")

    def expect_profile_dev(self, st, sq, mode, d_codes, d_profile, dtype, n_pos, d_off, d_len, n_rec, d_st, d_sq, d_occ, d_win):
        ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a)
        rc = self.L.pfmscan_expect_profile_dev(self.h, ptr(st), ptr(sq), st.shape[0], st.shape[1], mode, ptr(d_codes), ptr(d_profile), dtype, n_pos,
                                               ptr(d_off), ptr(d_len), n_rec, ptr(d_st), ptr(d_sq), ptr(d_occ), ptr(d_win))
        if rc != 0:
            raise RuntimeError("the baseline's pfmscan_expect_profile_dev returned %d" % rc)

    def synchronize(self):
        self.L.pfmscan_synchronize(self.h)

    def close(self):
        self.L.pfmscan_ctx_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--cases", default="8:1,12:1,18:1,12:256:4096", help="width:motifs[:records], comma separated")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-lib", default=None, help="libpfmscan.so of the commit before the table: route EP0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib
    n_all, L = args.records, args.length
    n_pos = n_all * (L + 1)
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    base = Baseline(args.baseline_lib) if args.baseline_lib else None
    own = Baseline(_lib.LIB_PATH) if base else None
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    codes = torch.randint(0, 4, (n_pos,), dtype=torch.uint8, device=dev, generator=g)
    codes.view(n_all, L + 1)[:, L] = 7
    prof = torch.rand((n_pos, 7), dtype=torch.float32, device=dev, generator=g)
    prof /= prof.sum(dim=1, keepdim=True)
    rec_off = torch.arange(n_all, dtype=torch.int64, device=dev) * (L + 1)
    rec_len = torch.full((n_all,), L, dtype=torch.int64, device=dev)
    windows = torch.empty(n_all, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(2)
    res = {"records": n_all, "length": L, "positions": n_pos, "rows": "float32", "iters": args.iters, "warmup": args.warmup,
           "device": ctx.device_info(), "baseline_lib": bool(base)}
    p = lambda t: t.data_ptr()
    for case in args.cases.split(","):
        part = [int(x) for x in case.split(":")]
        m, n_mo, n_rec = part[0], part[1], min(part[2], n_all) if len(part) > 2 else n_all
        S = np.ascontiguousarray(np.stack([struct_tables(rng, m)[1] for _ in range(n_mo)]))
        R = np.ascontiguousarray(np.stack([seq_table(rng, m) for _ in range(n_mo)]))
        occ = torch.empty((n_rec, n_mo), dtype=torch.float64, device=dev)
        e_st = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
        e_sq = torch.empty((n_rec, n_mo, m, 8), dtype=torch.float64, device=dev)
        e_jt = torch.empty((n_rec, n_mo, m, 4, 8), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        stream = (p(codes), p(prof), _lib.PROFILE_F32, n_pos, p(rec_off), p(rec_len), n_rec)

        def route_ep():
            ctx.expect_profile_dev(S, R, _lib.EXPECT_POSTERIOR, *stream, p(e_st), p(e_sq), p(occ), p(windows))

        def route_jm():
            ctx.expect_profile_joint_dev(S, R, _lib.EXPECT_POSTERIOR, *stream, p(e_st), p(e_sq), p(e_jt), p(occ), p(windows))

        def route_j():
            ctx.expect_profile_joint_dev(S, R, _lib.EXPECT_POSTERIOR, *stream, None, None, p(e_jt), p(occ), p(windows))

        def route_ep0():
            base.expect_profile_dev(S, R, _lib.EXPECT_POSTERIOR, *stream, p(e_st), p(e_sq), p(occ), p(windows))
            base.synchronize()                                           # its own context: its own stream

        def route_ep1():
            own.expect_profile_dev(S, R, _lib.EXPECT_POSTERIOR, *stream, p(e_st), p(e_sq), p(occ), p(windows))
            own.synchronize()

        calls = {"EP_margins": route_ep, "JM_table_and_margins": route_jm, "J_table_alone": route_j}
        if base:
            calls["EP0_margins_baseline_build"] = route_ep0
            calls["EP1_margins_this_build_own_context"] = route_ep1
        times = timed_alternating(ctx, calls, args.iters, args.warmup)
        entry = dict((name, spread(ms)) for name, ms in times.items())
        entry.update({"width": m, "motifs": n_mo, "records": n_rec, "table_bytes": e_jt.numel() * 8})
        ep = entry["EP_margins"]["median_ms"]
        entry["JM_over_EP"] = entry["JM_table_and_margins"]["median_ms"] / ep
        entry["J_over_EP"] = entry["J_table_alone"]["median_ms"] / ep
        if base:
            entry["EP_over_EP0"] = ep / entry["EP0_margins_baseline_build"]["median_ms"]
            entry["EP1_over_EP0"] = entry["EP1_margins_this_build_own_context"]["median_ms"] / entry["EP0_margins_baseline_build"]["median_ms"]
        # by the algorithm, per window: the table adds 28 m products and 28 m additions to level 0's 7 m + 7 m (+ 4 m additions)
        entry["by_count_JM_over_EP_level0"] = (18 * m + 56 * m) / (18.0 * m)
        bits = lambda: (int(e_st.view(torch.int64).sum()), int(e_sq.view(torch.int64).sum()))   # wrapping sums of the bit patterns
        of = []
        for route in (route_ep, route_jm) + ((route_ep0,) if base else ()):
            e_st.fill_(-1.0)
            e_sq.fill_(-1.0)
            torch.cuda.synchronize()
            route()
            ctx.synchronize()
            of.append(bits())
        entry["margins_bit_sums_equal_expect_profile_dev"] = of[1] == of[0]
        if base:
            entry["margins_bit_sums_equal_baseline_build"] = of[2] == of[0]
        entry["max_abs_diff_of_table_sum_over_nucleotides_to_exp_struct"] = float((e_jt.sum(dim=3) - e_st).abs().max())
        entry["all_finite"] = bool(torch.isfinite(e_jt).all())
        res["w%d_x%d" % (m, n_mo)] = entry
        del occ, e_st, e_sq, e_jt
        torch.cuda.empty_cache()
    if base:
        base.close()
        own.close()
    ctx.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
