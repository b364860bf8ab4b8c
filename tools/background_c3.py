"""Measurements of the profile column sums at C3 size (100k records x 3 kb): run under `rocprofv3 --kernel-trace --stats`
for the kernel times; prints HIP-event times of the same calls, the numpy time of the same sums on a sample,
and -- with --store DIR -- writes the float32 store the command-line timing reads and times numpy over it on 16 threads.

    python tools/background_c3.py [--records 100000] [--length 3000] [--iters 5] [--store DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def numpy_sums(store_dir, n_rec, L, threads, want):
    """the same per-record column sums with numpy over the mapped store (page cache warm: it was just written), ``threads``
    threads each taking whole records -> seconds; the sums must agree with the device's to the last few bits"""
    from concurrent.futures import ThreadPoolExecutor
    rows = np.memmap(os.path.join(store_dir, "profile.f32"), dtype=np.float32, mode="r", shape=(n_rec, L + 1, 7))
    step = 500
    out = np.empty((n_rec, 7), dtype=np.float64)

    def part(a):
        out[a:a + step] = rows[a:a + step].astype(np.float64).sum(axis=1)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(part, range(0, n_rec, step)))
    dt = time.perf_counter() - t0
    assert np.allclose(out, want, rtol=1e-12, atol=0)
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--store", default=None)
    ap.add_argument("--numpy-threads", type=int, default=16, help="with --store: threads of the numpy sums over the written store")
    args = ap.parse_args()
    import torch
    from rnascan_amd import _lib, store
    n_rec, L = args.records, args.length
    n_pos = n_rec * (L + 1)
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    off = torch.arange(n_rec, dtype=torch.int64, device=dev) * (L + 1)
    ln = torch.full((n_rec,), L, dtype=torch.int64, device=dev)
    out = torch.empty((n_rec, 7), dtype=torch.float64, device=dev)
    res = {"records": n_rec, "length": L, "rows": n_pos}
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    prof32 = torch.rand((n_pos, 7), dtype=torch.float32, device=dev, generator=g)
    prof32.view(n_rec, L + 1, 7)[:, L, :] = 0
    for name, prof in (("float32", prof32), ("float64", None)):
        if prof is None:
            prof = prof32.to(torch.float64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.profile_colsums_dev(prof.data_ptr(), np.float32 if name == "float32" else np.float64, n_pos, off.data_ptr(),
                                ln.data_ptr(), n_rec, out.data_ptr())
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            e0.record()
            ctx.profile_colsums_dev(prof.data_ptr(), np.float32 if name == "float32" else np.float64, n_pos, off.data_ptr(),
                                    ln.data_ptr(), n_rec, out.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        nbytes = prof.numel() * prof.element_size()
        res[name] = {"bytes": nbytes, "call_ms_min": min(times), "call_ms": times, "TB_per_s_at_min": nbytes / min(times) / 1e9}
        if name == "float32":
            sample = prof[: 2000 * (L + 1)].cpu().numpy()
            t0 = time.perf_counter()
            cpu = sample.reshape(2000, L + 1, 7).astype(np.float64).sum(axis=1)
            dt = time.perf_counter() - t0
            res["numpy_one_thread_s_for_all_records"] = dt * n_rec / 2000
            got = out[:2000].cpu().numpy()
            res["max_rel_diff_vs_numpy_sample"] = float(np.abs(got - cpu).max() / cpu.max())
            if args.store:
                os.makedirs(args.store, exist_ok=True)
                with open(os.path.join(args.store, "profile.f32"), "wb") as f:
                    for a in range(0, n_pos, 1 << 24):
                        f.write(prof[a:a + (1 << 24)].cpu().numpy().tobytes())
                store.write_index(args.store, ["r%d" % i for i in range(n_rec)], [L] * n_rec, list("BEHLMRT"), np.float32, "profile.f32")
                res["numpy_%d_threads_s" % args.numpy_threads] = numpy_sums(args.store, n_rec, L, args.numpy_threads, out.cpu().numpy())
        del prof
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
