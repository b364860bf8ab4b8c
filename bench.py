#!/usr/bin/env python3
"""bench.py -- scored windows/s of the seq+struct sliding-window scan (w=12) on MI355X.

Workload (BASELINE.json configs[2], "C3"): 100k synthetic RNA records x 3 kb,
uint8 letter codes + averaged-structure profile (7 x float32 per position),
sequence PFM and structure PFM of width 12, all-scores mode (one float32 sequence
score + one float64 structure score per window).  A "step" is ONE pass of the hot
path over the whole batch, inputs already resident in HBM.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR     # + the last step's outputs as DIR/*.npy
    python bench.py --gpus 1 --steps 20 --warmup 3 --full                 # + baselines, floors, parity, secondary legs
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Multi-GPU: records are independent, so every rank scans its own
shard (weak scaling), no data-path collective; only the timing barrier and a MAX
over ranks use RCCL.  With 8 ranks the default shard is 125k records: BASELINE
configs[3] ("C4": 1M records x 3 kb over 8 GPUs); the line then carries every rank's
kernel time and (--full) a per-rank parity sample against the CPU oracle.

Prints ONE JSON line (rank 0).  ``roofline`` is computed from the ALGORITHMIC
bytes (29 B read per position + 12 B written per window)
and the average kernel duration measured with HIP events on the launch stream.

A plain run does only what that line needs: set up, settle and warm up, time the
steps, write --dump-outputs, print.  ``--full`` adds what takes runs of its own
after the timed region: the same kernel on default-allocator arrays, this GPU's
live memory floor (tools/hbm_mixed), the per-rank parity sample of multi-GPU runs,
``cpu_baseline`` (the CPU oracle, oracle/pfm_oracle.c with OpenMP, on a bounded
sample of the same records on this box's host cores, the same sample used as a
parity check of the GPU scores), the reference-structured baseline and the
secondary legs (bench_legs.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from bench_legs import (HBM_PEAK_GBS, combined_threshold, library_roofline, live_mixed_floor, make_pssms, make_stream,  # noqa: E402
                        pmc_entry, probe_motifs, secondary_legs, struct_only_threshold, timed)



def dry_run(args, world):
    """PFMSCAN_BENCH_DRYRUN=1: the multi-rank plumbing WITHOUT the hot path -- rank environment, process group (gloo),
    barrier, MAX over ranks, per-rank gather, rank 0's line -- for the launcher test on a machine without a GPU.  No
    score is computed and no throughput is reported (value = null, "dry_run": true); a "step" is a 1 ms host sleep."""
    rank = int(os.environ.get("RANK", "0"))
    if os.environ.get("PFMSCAN_BENCH_DRYRUN_FAIL_RANK") == str(rank):
        raise SystemExit(3)                       # the launcher test's failing rank
    # the shard arithmetic of the real run (weak scaling: fixed work per GPU; C4 = 8 x 125 000 records of 3 kb)
    records = args.records if args.records is not None else (125000 if world == 8 else 100000)
    windows = records * (args.length - args.width + 1) * (args.motifs if args.workload in ("c5", "c5s") else 1)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001)
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    kernel_ms = elapsed / args.steps * 1e3
    rank_ms = [kernel_ms]
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0])
        box = [None] * world
        dist.all_gather_object(box, (kernel_ms, records, windows, rank))
        rank_ms = [b[0] for b in box]
        assert [b[3] for b in box] == list(range(world))
        all_windows = sum(b[2] for b in box)
        all_records = sum(b[1] for b in box)
    else:
        all_windows, all_records = windows, records
    result = None
    if rank == 0:
        shard = "C4: 1M records x 3 kb over 8 GPUs" if (world == 8 and records == 125000 and args.length == 3000) else "%d x %d records" % (world, records)
        result = {"metric": "DRY RUN of the multi-rank launcher (no GPU work, no score computed)", "value": None, "unit": "windows/s",
                  "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
                  "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "none", "dry_run": True,
                  "config": {"workload": "none (PFMSCAN_BENCH_DRYRUN=1); the real run would scan " + shard, "bench_workload": args.workload,
                             "records_per_gpu": records, "records_all_ranks": all_records, "record_length": args.length,
                             "pfm_width": args.width, "windows_per_gpu_per_step": windows, "windows_all_ranks_per_step": all_windows,
                             "sharding": "records, no collective"},
                  # what `value` is made of in the real run: the units ALL ranks processed / the slowest rank's time
                  "value_formula": "windows_all_ranks_per_step * steps / (MAX over ranks of the timed region)",
                  "per_rank": {"kernel_ms": rank_ms}}
        print(json.dumps(result))
        sys.stdout.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return result


DUMP_BYTES = 48 << 20          # --dump-outputs: what one run writes at most (all ranks together), headers and indices aside
DUMP_SEED = 20240601           # the record sample of --dump-outputs


def dump_sample_records(records, k):
    """the fixed, seeded, sorted sample of k of `records` record indices that --dump-outputs keeps (all when k >= records)"""
    if k >= records:
        return np.arange(records, dtype=np.int64)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(records, size=max(1, k), replace=False)).astype(np.int64)


def collect_outputs(torch, dev, args, world, stride, out_seq, out_st, hits):
    """--dump-outputs: what the timed path handed its caller in the LAST timed step, as float32 / float64 host arrays.

    all-scores modes: the window scores (float32 sequence, float64 structure) of the records of dump_sample_records(), the
    budget deciding how many, as [records kept, length - width + 1] rows: the windows that lie inside a record.  The
    stream's other positions (a window over the record's end and its separator) hold no window; they are left out.
    hits modes: the hits sorted by (position, motif) -- the device entry points append them in no particular order --
    with the position (and motif index) as float64; when they exceed the budget, only those that start in the records of
    dump_sample_records() (a share of the records the size of the budget's share of the hits) are kept."""
    budget = DUMP_BYTES // world
    out = {}
    if hits is None:
        n_win = args.length - args.width + 1
        per_record = n_win * (4 + (8 if out_st is not None else 0))
        rec = dump_sample_records(args.records, budget // per_record)
        idx = (torch.from_numpy(rec).to(dev)[:, None] * stride + torch.arange(n_win, device=dev)[None, :]).reshape(-1)
        out["record_index"] = rec.astype(np.float64)
        out["scores_seq"] = out_seq[idx].cpu().numpy().reshape(len(rec), n_win)
        if out_st is not None:
            out["scores_struct"] = out_st[idx].cpu().numpy().reshape(len(rec), n_win)
        return out
    total, pos, motif, sq, st = hits
    order = np.lexsort((motif, pos)) if motif is not None else np.argsort(pos, kind="stable")
    cols = {"hit_pos": pos, "hit_motif": motif, "hit_seq": sq, "hit_struct": st}
    cols = {k: v[order] for k, v in cols.items() if v is not None}
    per_hit = sum(8 if k != "hit_seq" else 4 for k in cols)
    if len(pos) * per_hit > budget:
        rec = dump_sample_records(args.records, args.records * budget // (len(pos) * per_hit))
        keep = np.isin(cols["hit_pos"] // stride, rec)
        hard = budget * 5 // 4 // per_hit                     # hits crowded into the sampled records: the first ones only
        cols = {k: v[keep][:hard] for k, v in cols.items()}
        out["record_index"] = rec.astype(np.float64)
    out["hit_count"] = np.array([total], dtype=np.float64)
    for k, v in cols.items():
        out[k] = v.astype(np.float32 if k == "hit_seq" else np.float64)
    return out


def write_outputs(outdir, arrays, rank, world):
    os.makedirs(outdir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(outdir, ("rank%d_%s.npy" % (rank, name)) if world > 1 else name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="GPUs of this node to run on [1].  Under a launcher (WORLD_SIZE set, e.g. torch.distributed.run "
                         "--nproc-per-node N) it must equal WORLD_SIZE; without one, N > 1 makes this process the parent of N "
                         "ranks (rnascan_amd/launch.py: it never touches a GPU itself) and relays rank 0's JSON line")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=15,
                    help="untimed launches right after data generation, BEFORE the --warmup steps: the chip's clocks "
                         "take ~10 launches to settle after the generation kernels (per-dispatch times ramp 3.1 -> 2.3 ms)")
    ap.add_argument("--records", type=int, default=None,
                    help="records per GPU [100000; 125000 with 8 GPUs = C4: 1M records over the node]")
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--width", type=int, default=12)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure and check what the headline does not need: the same kernel on "
                         "default-allocator arrays, the live memory floor, the per-rank parity sample, the CPU baselines with "
                         "their parity check and the secondary legs.  The --no-* options below leave parts of it out")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target CPU work for the cpu_baseline sample (--full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines and the parity checks against the oracle")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full without the secondary legs (C5, its structure-only form and C2 hits on the resident "
                         "stream, after the headline's timed region)")
    ap.add_argument("--no-ref-structured", action="store_true",
                    help="--full without the reference-structured Python baseline (B-ref of BASELINE.md section 3)")
    ap.add_argument("--workload", choices=["c3", "c2", "c5", "c5s"], default="c3",
                    help="c3: seq+struct w=12 (the headline metric); c2: sequence-only PFM (BASELINE configs[1], use --width 8); "
                         "c5: a library of --motifs seq+struct PFM pairs over the same resident records, every motif in ONE "
                         "pass of the library kernel, thresholded hits (BASELINE configs[4]); value is then window x motif "
                         "pairs per second; c5s: the STRUCTURE-ONLY library of --motifs PFMs over the resident profile (k_profile_lib: "
                         "the profile is read once, bound by the fp64 vector rate)")
    ap.add_argument("--motifs", type=int, default=256, help="PFM pairs of --workload c5")
    ap.add_argument("--variant", choices=["finite", "inf"], default="finite",
                    help="finite: pseudocount 0.01 PSSMs (headline); inf: pseudocount 0 PSSMs with -inf cells, profile with "
                         "exact zeros and 0.1 %% foreign letters (exercises nan_to_num / NaN windows at full size)")
    ap.add_argument("--mode", choices=["scores", "hits", "hits2", "library"], default="scores",
                    help="scores: all-scores (the headline, 41.1 B/window); hits: thresholded hits, one fused pass "
                         "(29.1 B/window + 20 B/hit); hits2: candidate-then-verify (letters pass, structure only at its hits)")
    ap.add_argument("--profile-dtype", choices=["float32", "float64"], default="float32",
                    help="device storage of the profile rows (float32 = the headline, 41.1 B/window; float64 = the strict "
                         "variant of SURVEY 8d, 69.2 B/window)")
    ap.add_argument("--minscore", type=float, default=None,
                    help="one threshold for both sides (the reference's -m): seq > m and struct > m; overrides the two below")
    ap.add_argument("--minscore-seq", type=float, default=6.0, help="sequence threshold of the hits modes [the CLI's default -m 6]")
    ap.add_argument("--minscore-struct", type=float, default=None,
                    help="structure threshold of the hits modes [auto: the quantile of the structure scores of the windows "
                         "passing the sequence threshold that gives a combined hit rate of --hit-rate]")
    ap.add_argument("--from-host", action="store_true",
                    help="END-TO-END line instead of the device-resident one: the packed stream starts in pageable host memory "
                         "(as a memory-mapped profile store does); a step = pfmscan_hits_pipeline_host: chunked upload on a copy "
                         "stream beside the scan of the previous chunk, hits sorted and copied back.  Reports windows/s and the "
                         "PCIe rate; never the headline value")
    ap.add_argument("--chunk-positions", type=int, default=1 << 24, help="chunk of --from-host (stream positions)")
    ap.add_argument("--placement", choices=["tuned", "plain", "torch"], default="tuned",
                    help="where the resident arrays (codes, profile, both score arrays) lie in HBM.  tuned: pfmscan_place_alloc -- the "
                         "library takes chunks of device memory, measures which disturb each other (shared DRAM banks) and gives the arrays "
                         "of the scan chunks that do not (DESIGN.md section 3; the same kernel runs 2.2 ms or 1.96 ms depending on this); plain: "
                         "the same allocator without the measurement; torch: torch's caching allocator, wherever that puts them")
    ap.add_argument("--hit-rate", type=float, default=1e-4, help="target combined hit rate of the auto structure threshold (SURVEY 8d C5)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (float32 / float64, at most "
                         "48 MB over all ranks: a fixed, seeded sample of records when the outputs are larger; all-scores runs "
                         "write the windows inside the records; with N ranks the "
                         "names start with rank<k>_).  The inputs depend on the arguments alone, so two builds can be compared "
                         "output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.minscore is not None:
        args.minscore_seq = args.minscore_struct = args.minscore
    if args.from_host and args.mode == "scores":
        args.mode = "hits"
    # ---- N GPUs from one command: the parent starts N ranks BEFORE anything here touches a GPU (no torch.cuda call, no
    # _lib.Context), waits, and prints what rank 0 printed; a failing rank makes it exit non-zero
    from rnascan_amd import launch
    world, must_spawn = launch.resolve_world(args.gpus)
    if must_spawn:
        rc, text = launch.spawn_ranks(world, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:], capture_rank0=True)
        for ln in (text or "").splitlines():     # stdout = the result line only; anything else rank 0 printed goes to stderr
            (sys.stdout if ln.startswith("{") else sys.stderr).write(ln + "\n")
        sys.stdout.flush()
        if rc == 0 and not any(ln.startswith("{") and '"n_gpus": %d' % world in ln for ln in (text or "").splitlines()):
            sys.stderr.write("bench.py: rank 0 printed no result line for %d GPUs\n" % world)
            rc = 1
        sys.exit(rc)
    if os.environ.get("PFMSCAN_BENCH_DRYRUN") == "1":
        return dry_run(args, world)
    # the cpu_baseline leg uses every logical CPU this process may run on (north_star: "all host cores").  libgomp reads
    # OMP_NUM_THREADS when it is LOADED (torch loads it), and its own default stops at 128 of this box's 256 CPUs.
    os.environ.setdefault("OMP_NUM_THREADS", str(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()))

    import torch
    from rnascan_amd import _lib

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.records is None:
        args.records = 125000 if world == 8 else 100000
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (libpfmscan has no CPU fallback)")
    # rehearsal on a one-GPU box: PFMSCAN_BENCH_REHEARSE=1 puts every rank on device 0 and rendezvous over gloo
    # (RCCL refuses two ranks on one device); the product launch is one rank per GPU over RCCL
    rehearse = os.environ.get("PFMSCAN_BENCH_REHEARSE") == "1"
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    # PFMSCAN_BENCH_FORCE_DIST=1 (under torchrun --nproc-per-node 1): the RCCL process group, barrier, MAX reduction and
    # object gather of the multi-GPU path with ONE rank -- the only way to run that code on a one-GPU box
    if world > 1 or os.environ.get("PFMSCAN_BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    ctx = _lib.Context(local_rank)
    table, spssm = make_pssms(args.width, args.variant)
    seq_only = args.workload == "c2"
    struct_lib = args.workload == "c5s"
    is_lib = args.workload in ("c5", "c5s")
    motif = ctx.motif(table, None if seq_only else spssm)
    library = None
    if is_lib:
        args.mode = "library"
        tabs = [make_pssms(args.width, args.variant, seed=1000 + k) for k in range(args.motifs)]      # seeds 1000 + k
        lib_T, lib_P = np.stack([t for t, _ in tabs]), np.stack([p for _, p in tabs])
        library = ctx.library(None if struct_lib else lib_T, lib_P)
    # the resident arrays, placed BEFORE anything else takes device memory (more candidates to choose from)
    n_pos = args.records * (args.length + 1)
    prow = 7 * (8 if args.profile_dtype == "float64" else 4)
    placed, placement = None, {"mode": "torch"}
    if args.placement != "torch" and not args.from_host:
        try:
            t_pl = time.perf_counter()
            placed = ctx.place_alloc([n_pos * prow, n_pos * 8, n_pos * 4, n_pos], plain=args.placement == "plain")
            placement = {"mode": args.placement, "seconds": round(time.perf_counter() - t_pl, 3), "note": ctx.place_note()}
        except Exception as exc:                     # e.g. no virtual memory API on this driver: the arrays come from torch instead
            placement = {"mode": "torch", "note": "pfmscan_place_alloc failed (%s); torch's allocator was used" % exc}
    codes, profile, n_pos = make_stream(torch, dev, args.records, args.length, 20240601 + rank,
                                        foreign=0.001 if args.variant == "inf" else 0.0,
                                        zero_snap=args.variant == "inf")
    ptype = _lib.PROFILE_F32
    if args.profile_dtype == "float64":
        profile = profile.double()
        ptype = _lib.PROFILE_F64
    if placed is not None:
        raw = [torch.as_tensor(a, device=dev) for a in placed]          # uint8 views of the placed ranges, no copy
        assert all(t.data_ptr() == a.ptr for t, a in zip(raw, placed))
        p_new = raw[0].view(profile.dtype).view(n_pos, 7)
        p_new.copy_(profile)
        c_new = raw[3]
        c_new.copy_(codes)
        del profile, codes
        torch.cuda.empty_cache()
        profile, codes = p_new, c_new
        out_st, out_seq = raw[1].view(torch.float64), raw[2].view(torch.float32)
        out_st.zero_()
        out_seq.zero_()
    else:
        # zero-filled (touched) outputs: first-touch of fresh device pages would otherwise
        # land in the first kernel launches and skew the per-kernel average rocprof reports
        out_seq = torch.zeros(n_pos, dtype=torch.float32, device=dev)
        out_st = torch.zeros(n_pos, dtype=torch.float64, device=dev)
    windows = args.records * (args.length - args.width + 1)
    # a real (non-null) torch stream: the ABI reads stream NULL as "the ctx's own
    # stream", and the HIP events below must sit on the stream the kernel runs on
    torch.cuda.synchronize()                 # generation ran on the default stream: finish it first
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    assert stream != 0

    # ---- thresholds of the hits modes: the CLI's default -m 6 on the sequence side; the structure threshold, unless
    # given, is the quantile that makes the COMBINED hit rate --hit-rate ("threshold chosen for ~1e-4"), so
    # that hit emission, the sharded counters and (library) the structure verification all carry real load
    thr_seq, thr_struct, thr_note = args.minscore_seq, args.minscore_struct, "given"
    rate_seq = None
    if struct_lib and thr_struct is None:
        thr_struct, thr_note = struct_only_threshold(torch, ctx, tabs, profile, ptype, n_pos, out_st, stream, args.hit_rate)
    if args.mode != "scores" and not seq_only and thr_struct is None:
        probe = [ctx.motif(*tp) for tp in probe_motifs(tabs)] if is_lib else [motif]
        thr_struct, rate_seq, thr_note = combined_threshold(torch, ctx, probe, codes, profile, ptype, n_pos, out_seq, out_st, stream,
                                                            windows, thr_seq, args.hit_rate)
        if is_lib:
            for m0 in probe:
                m0.close()
    if seq_only or thr_struct is None:
        thr_struct = -np.inf if seq_only else thr_struct

    cap = 1 << 25 if is_lib else 1 << 24
    if args.mode != "scores":
        hit_pos = torch.empty(cap, dtype=torch.int64, device=dev)
        hit_motif = torch.empty(cap if is_lib else 1, dtype=torch.int32, device=dev)
        hit_seq = torch.empty(cap, dtype=torch.float32, device=dev)
        hit_st = torch.empty(cap, dtype=torch.float64, device=dev)
        hit_count = torch.zeros(1, dtype=torch.int64, device=dev)

    host_hits = [0, None]
    if args.from_host:
        codes_h = codes.cpu().numpy()
        profile_h = None if seq_only else profile.cpu().numpy()

    def step():
        if args.from_host:
            pos, sq, st = ctx.hits_pipeline_host(motif, codes_h, profile_h, thr_seq, thr_struct, args.chunk_positions)
            host_hits[0], host_hits[1] = len(pos), (pos, sq, st)
            return
        if is_lib:
            ctx.library_hits_dev(library, None if struct_lib else codes.data_ptr(), profile.data_ptr(), ptype, n_pos,
                                 None if struct_lib else thr_seq, thr_struct, cap, hit_pos.data_ptr(), hit_motif.data_ptr(),
                                 None if struct_lib else hit_seq.data_ptr(), hit_st.data_ptr(), hit_count.data_ptr(), stream)
        elif args.mode in ("hits", "hits2"):
            hit_count.zero_()
            (ctx.hits_dev if args.mode == "hits" else ctx.hits_adaptive_dev)(
                motif, codes.data_ptr(), None if seq_only else profile.data_ptr(), _lib.PROFILE_NONE if seq_only else ptype,
                n_pos, thr_seq, thr_struct, cap, hit_pos.data_ptr(), hit_seq.data_ptr(), hit_st.data_ptr(),
                hit_count.data_ptr(), stream)
        elif seq_only:
            ctx.scan_dev(motif, codes.data_ptr(), None, _lib.PROFILE_NONE, n_pos, out_seq.data_ptr(), None, stream)
        else:
            ctx.scan_dev(motif, codes.data_ptr(), profile.data_ptr(), ptype, n_pos,
                         out_seq.data_ptr(), out_st.data_ptr(), stream)

    def barrier():
        if dist is not None:
            dist.barrier()

    # settle: untimed launches until the clocks have ramped -- at least --settle of them AND at least 40 ms of
    # them (15 launches of the 0.3 ms sequence-only kernel are over before the ramp is: C2 read 0.33 ms with
    # them and 0.29 ms in steady state)
    settled = 0
    t_s = time.perf_counter()
    while settled < (2 if is_lib else args.settle) or (time.perf_counter() - t_s < 0.040 and settled < 5000):
        step()
        settled += 1
        if settled >= args.settle and settled % 16 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    # one HIP event per step boundary, on the launch stream: the per-step durations give median / min / max over
    # exactly the timed dispatches (directly comparable with a rocprofv3 kernel trace of the same steps)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(args.steps):
        step()
        evs[i + 1].record()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    step_ms = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)])
    kernel_ms = float(evs[0].elapsed_time(evs[args.steps]) / args.steps)          # HIP events on the launch stream
    kernel_ms_rank = kernel_ms
    n_hits = None
    if args.mode != "scores":
        n_hits = host_hits[0] if args.from_host else int(hit_count.item())
    if args.dump_outputs:
        hits = None
        if args.from_host:
            pos, sq, st = host_hits[1]
            hits = (n_hits, pos, None, sq, st)
        elif args.mode != "scores":
            k = min(n_hits, cap)
            hits = (n_hits, hit_pos[:k].cpu().numpy(), hit_motif[:k].cpu().numpy() if is_lib else None,
                    None if struct_lib else hit_seq[:k].cpu().numpy(), None if seq_only else hit_st[:k].cpu().numpy())
        write_outputs(args.dump_outputs, collect_outputs(torch, dev, args, world, args.length + 1, out_seq,
                                                         None if seq_only else out_st, hits), rank, world)

    # ---- the same kernel on arrays from the DEFAULT allocator (what callers that do not use pfmscan_place_alloc get), after
    # the timed region and under the same clocks: the line carries both, so the kernel's share and the placement's share of
    # the headline can be told apart in one record
    default_alloc = None
    # (not under a profiler: the kernel trace's average for this kernel is compared with `kernel_ms`, which times the placed arrays)
    under_profiler = "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or \
        bool(os.environ.get("PFMSCAN_BENCH_NO_FLOOR"))
    if (args.full and placed is not None and args.mode == "scores" and not is_lib and not os.environ.get("PFMSCAN_BENCH_NO_DEFAULT_ALLOC")
            and not under_profiler):
        try:
            d_codes, d_prof = codes.clone(), (None if seq_only else profile.clone())
            d_seq, d_st = torch.zeros(n_pos, dtype=torch.float32, device=dev), (None if seq_only else torch.zeros(n_pos, dtype=torch.float64, device=dev))

            def step_default():
                ctx.scan_dev(motif, d_codes.data_ptr(), None if seq_only else d_prof.data_ptr(), _lib.PROFILE_NONE if seq_only else ptype, n_pos,
                             d_seq.data_ptr(), None if seq_only else d_st.data_ptr(), stream)
            for _ in range(5):
                step_default()
            torch.cuda.synchronize()
            dev_evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            dev_evs[0].record()
            for i in range(args.steps):
                step_default()
                dev_evs[i + 1].record()
            torch.cuda.synchronize()
            d_ms = np.array([dev_evs[i].elapsed_time(dev_evs[i + 1]) for i in range(args.steps)])
            default_alloc = {"kernel_ms": float(dev_evs[0].elapsed_time(dev_evs[args.steps]) / args.steps),
                             "kernel_ms_median": float(np.median(d_ms)), "kernel_ms_min": float(d_ms.min())}
            del d_codes, d_prof, d_seq, d_st
            torch.cuda.empty_cache()
        except Exception as exc:                                  # e.g. not enough memory for a second resident set
            default_alloc = {"error": str(exc)}

    # ---- this rank's memory floor (tools/hbm_mixed on THIS rank's GPU): a slow rank and a badly placed one look different
    rank_floor = None
    if args.full and not is_lib and args.mode == "scores" and (seq_only or args.profile_dtype == "float32") and not args.from_host:
        # one rank after the other: the tool is a child process on the rank's GPU, and a node should never see more than ONE extra
        # process beside the N ranks (process limits of shared boxes), nor two floors disturbing each other's memory traffic
        for turn in range(world):
            if turn == rank:
                rank_floor = live_mixed_floor(args.records, args.length, placed=placed is not None and args.placement == "tuned",
                                              device=local_rank, c2=seq_only)
            if dist is not None:
                dist.barrier()

    # ---- per-rank parity sample (multi-GPU runs): a few records of THIS rank's shard against the CPU oracle
    rank_parity = None
    if args.full and dist is not None and args.mode == "scores" and not seq_only and not args.no_cpu_baseline:
        from oracle import oracle
        if rank == 0:
            oracle.build()                   # one rank compiles (when stale at all), the others load the finished library
        barrier()
        stride = args.length + 1
        nrec = min(args.records, 8)
        c = codes[: nrec * stride].cpu().numpy()
        pr = profile[: nrec * stride].cpu().numpy()
        ref_seq, ref_st = oracle.stream_seq(c, table), oracle.stream_struct(pr, spssm)
        got_seq, got_st = out_seq[: nrec * stride].cpu().numpy(), out_st[: nrec * stride].cpu().numpy()
        v = ~np.isnan(ref_seq)
        ok_seq = bool(np.array_equal(np.isnan(got_seq), ~v) and np.array_equal(got_seq[v].view(np.uint32), ref_seq[v].view(np.uint32)))
        vs = np.isfinite(ref_st) & (np.abs(ref_st) < 1e9)
        rank_parity = bool(ok_seq and float(np.abs(got_st[vs] - ref_st[vs]).max()) <= 1e-6)

    rank_ms, rank_ok, rank_hits, rank_detail = [kernel_ms], [rank_parity], [n_hits], {}
    if dist is not None:
        t = torch.tensor([elapsed, kernel_ms], dtype=torch.float64, device="cpu" if rehearse else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, kernel_ms = float(t[0]), float(t[1])
        box = [None] * world
        dist.all_gather_object(box, (kernel_ms_rank, rank_parity, n_hits, float(np.median(step_ms)), float(step_ms.min()), placement.get("note"),
                                     default_alloc, rank_floor))
        rank_ms, rank_ok, rank_hits = [b[0] for b in box], [b[1] for b in box], [b[2] for b in box]
        rank_detail = {"kernel_ms_median": [b[3] for b in box], "kernel_ms_min": [b[4] for b in box], "placement_note": [b[5] for b in box],
                       "kernel_ms_default_allocator": [None if not b[6] else b[6].get("kernel_ms") for b in box],
                       "mixed_read_write_floor_ms": [None if not b[7] else b[7]["ms"] for b in box]}

    result = None
    if rank == 0:
        n_motifs = args.motifs if is_lib else 1
        total_windows = windows * world * args.steps * n_motifs
        in_b, out_b, hit_b = (1, 4, 12) if seq_only else (29 if ptype == _lib.PROFILE_F32 else 57, 12, 20)
        alg_bytes = args.records * args.length * in_b + windows * out_b      # per launch, per GPU
        if args.mode != "scores":
            alg_bytes = args.records * args.length * in_b + min(n_hits, cap) * hit_b
        achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
        traffic, traffic_source = None, None
        tfile = os.path.join(REPO, "profiles", "pmc_traffic.json")
        if os.path.exists(tfile) and args.mode == "scores" and args.profile_dtype == "float32":
            try:
                tj_all = json.load(open(tfile))
                for tj in tj_all.get("entries", []):
                    if (tj.get("workload") == args.workload and tj.get("records") == args.records
                            and tj.get("length") == args.length and tj.get("width") == args.width):
                        traffic = tj.get("hbm_bytes_per_launch")
                        traffic_source = "profiles/pmc_traffic.json (%s; rocprofv3 --pmc passes of %s, not measured in this run)" % (
                            tj.get("kernel", "?"), tj.get("date", tj_all.get("date", "?")))
            except Exception:
                traffic = None
        shard = "C4: 1M" if (world == 8 and args.records == 125000) else "%d x %d" % (world, args.records)
        if struct_lib:
            wl = ("C5-struct: library of %d structure PFMs (width %d) x %d synthetic records x %d nt per GPU, resident %s profile, "
                  "every motif in ONE pass over the profile (k_profile_lib: tile rows staged in LDS as fp64 once, PSSM rows through "
                  "the scalar cache), thresholded hits per motif" % (n_motifs, args.width, args.records, args.length, args.profile_dtype))
        elif is_lib:
            wl = ("C5: library of %d seq+struct PFM pairs (width %d) x %d synthetic records x %d nt per GPU, resident stream, "
                  "every motif in one pass (k_library: integer two-letter prefilter in LDS, exact re-score + structure "
                  "verification of the survivors), thresholded hits per motif" % (n_motifs, args.width, args.records, args.length))
        elif seq_only:
            wl = "C2: %d synthetic RNA records x %d nt per GPU, sequence PFM width %d, uint8 codes" % (args.records, args.length, args.width)
        else:
            wl = ("%s: %d synthetic RNA records x %d nt per GPU, seq PFM + averaged-structure PFM width %d, uint8 codes + %s "
                  "[n][7] profile, %s" % ("C4 (1M records x 3 kb over 8 GPUs)" if shard.startswith("C4") else
                                          ("C4 (1M records x 3 kb), all of it resident on each GPU" if args.records == 1000000 else "C3"), args.records,
                                          args.length, args.width, args.profile_dtype,
                                          "all-scores (f32 seq + f64 struct per window)" if args.mode == "scores" else "thresholded hits"))
        result = {
            "metric": ("scored window x motif pairs/sec (%d-PFM library, %s, w=%d)" % (n_motifs, "struct-only" if struct_lib else "seq+struct", args.width)) if is_lib
                      else "scored windows/sec (%s, w=%d)" % ("seq-only" if seq_only else "seq+struct", args.width),
            "value": total_windows / elapsed,
            "unit": "window-motif pairs/s" if is_lib else "windows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": wl,
                "records_per_gpu": args.records, "record_length": args.length, "pfm_width": args.width,
                "variant": args.variant, "settle_launches": settled, "windows_per_gpu_per_step": windows,
                "mode": {"scores": "all-scores", "library": "library hits"}.get(args.mode, "hits"),
                "minscore_seq": None if args.mode == "scores" else thr_seq,
                "minscore_struct": None if (args.mode == "scores" or seq_only) else thr_struct,
                "minscore_struct_source": None if (args.mode == "scores" or seq_only) else thr_note,
                "hits_per_step": n_hits, "hits_per_step_all_ranks": sum(h for h in rank_hits if h is not None) if n_hits is not None else None,
                "hit_rate": None if n_hits is None else n_hits / (windows * n_motifs),
                "sharding": "records, no collective",
                "placement": placement,
            },
            "roofline": {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                "kernel": ("k_letters_pre" if args.mode != "scores" else ("k_letters_fixed" if 2 <= args.width <= 32 and not os.environ.get("PFMSCAN_LETTERS_GENERIC") else "k_letters")) if seq_only else (
                    "k_profile_fixed" if (args.mode in ("scores", "hits") and 9 <= args.width <= 18 and not os.environ.get("PFMSCAN_PROFILE_GENERIC")) else "k_profile"),
                "kernel_ms": kernel_ms, "kernel_ms_median": float(np.median(step_ms)), "kernel_ms_min": float(step_ms.min()),
                "kernel_ms_max": float(step_ms.max()), "algorithmic_bytes_per_launch": alg_bytes,
                "frac_of_measured_copy_peak_6290": achieved / 6290.0,
            },
        }
        if seq_only and args.mode == "scores" and rank_floor is not None:
            # C2's byte mix (1 B read + 4 B written per position) moved by a program that scores nothing: tools/hbm_mixed ... c2
            result["roofline"]["mixed_read_write_floor"] = dict(rank_floor, frac_of_floor=rank_floor["ms"] / kernel_ms,
                                                                kernel_over_floor=kernel_ms / rank_floor["ms"])
        if not seq_only and not is_lib and args.mode == "scores" and args.profile_dtype == "float32":
            # the same byte mix (29 B in + 12 B out per position) moved by a program that scores nothing
            # (tools/hbm_mixed.hip, measured on this chip in round 4): what the memory system gives this access pattern
            live = rank_floor
            floor = pmc_entry("c3_mixed_floor")
            if live is not None:
                result["roofline"]["mixed_read_write_floor"] = dict(live, frac_of_floor=live["ms"] / kernel_ms, kernel_over_floor=kernel_ms / live["ms"])
            elif floor.get("records") == args.records and floor.get("length") == args.length:
                result["roofline"]["mixed_read_write_floor"] = {
                    "ms": floor["floor_ms"], "tb_per_s": floor["floor_tb_per_s"], "frac_of_floor": floor["floor_ms"] / kernel_ms,
                    "source": floor["source"], "note": "stored measurement of tools/hbm_mixed (its fastest form) on ANOTHER box, not taken in this run "
                                                       "(--full takes it live where tools/hbm_mixed is built): boxes differ by up to 10 % on it"}
        if traffic is not None:
            result["roofline"]["traffic_pmc_round"] = pmc_entry("c2" if seq_only else "c3").get("round")
        if default_alloc is not None:
            result["roofline"]["kernel_ms_default_allocator"] = default_alloc.get("kernel_ms")
            result["roofline"]["default_allocator"] = dict(default_alloc, frac=None if "kernel_ms" not in default_alloc else
                                                           alg_bytes / (default_alloc["kernel_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                           note="the same kernel, the same data, arrays from torch's caching allocator (hipMalloc) instead of "
                                                                "pfmscan_place_alloc; measured right after the timed region")
        if dist is not None:
            result["per_rank"] = dict({"kernel_ms": rank_ms, "parity_sample_ok": rank_ok,
                                       "note": "no 1 -> N curve is claimed by this line: value = all ranks' windows / max-over-ranks time"},
                                      **rank_detail)
        if args.from_host:
            h2d = args.records * (args.length + 1) * in_b
            result["metric"] = "END-TO-END " + result["metric"] + " from pageable host memory (upload + scan + sorted hits back)"
            result["roofline"] = None
            result["host_path"] = {
                "entry_point": "pfmscan_hits_pipeline_host", "chunk_positions": args.chunk_positions,
                "h2d_bytes_per_step": h2d, "pcie_gbs": h2d / (elapsed / args.steps) / 1e9,
                "pcie_reference_gbs": {"gen5_x16_spec": 63.0, "r1_stage_probe_measured": 56.0},
                "note": "a step is bounded by the host-to-device copy; the device-resident kernel rate is the headline bench line",
            }
        if args.mode == "hits2":
            # candidate-then-verify reads 1 B per position plus m rows per candidate: the fused-pass byte
            # count does not describe it, so no roofline figure is given for this mode
            result["roofline"] = None
        if struct_lib:
            # bound by the fp64 vector rate: 7 m FMAs per window and motif; v_fma_f64 measured at 36.5 T lane-ops/s = 73 TFLOP/s
            # (tools/fp64_peak.hip, profiles/r1/fp64_peak.txt; the datasheet's 78.6 TFLOP/s is the same rate at 2.4 GHz)
            flops = float(windows) * n_motifs * args.width * 7 * 2
            tf = flops / (kernel_ms * 1e-3) / 1e12
            result["roofline"] = {
                "bound": "fp64", "achieved": tf, "peak": 73.0, "unit": "TFLOP/s", "frac": tf / 73.0, "traffic": None,
                "kernel": "k_profile_lib<%s>" % ("float" if ptype == _lib.PROFILE_F32 else "double"),
                "kernel_ms": kernel_ms, "kernel_ms_median": float(np.median(step_ms)), "kernel_ms_min": float(step_ms.min()),
                "kernel_ms_max": float(step_ms.max()), "algorithmic_flops_per_launch": flops,
                "algorithmic_unit": "fp64 FLOP: windows x motifs x 7 w FMAs x 2",
                "peak_source": "measured v_fma_f64 rate (profiles/r1/fp64_peak.txt); datasheet vector fp64 78.6 TFLOP/s",
                "frac_of_datasheet_78_6": tf / 78.6,
                "hbm_frac": (args.records * (args.length + 1) * (28 if ptype == _lib.PROFILE_F32 else 56) + (n_hits or 0) * 20)
                            / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            }
        elif is_lib:
            result["roofline"] = library_roofline(library.info(), windows, n_motifs, args.width, args.records, args.length, kernel_ms,
                                                  n_hits, rate_seq)
            result["roofline"].update({"kernel_ms_median": float(np.median(step_ms)), "kernel_ms_min": float(step_ms.min()),
                                       "kernel_ms_max": float(step_ms.max())})
        if args.full and dist is None and not args.no_cpu_baseline and args.mode == "scores" and not seq_only:
            usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
            from oracle import oracle
            oracle.build()
            stride = args.length + 1
            probe = min(args.records, 500)

            def cpu_run(nrec):
                c = codes[: nrec * stride].cpu().numpy()
                p = profile[: nrec * stride].cpu().numpy()
                t = time.perf_counter()
                s1 = oracle.stream_seq(c, table)
                s2 = oracle.stream_struct(p, spssm)
                return time.perf_counter() - t, s1, s2

            # thread count: every logical CPU the process may use is the upper end, but the box may give the job a smaller
            # CPU quota (cgroup cpu.max) and torch has set OpenMP to the physical core count -- so the probe is timed at
            # several counts and the FASTEST one runs the sample (the strongest honest CPU baseline)
            quota = None
            try:
                q, per = open("/sys/fs/cgroup/cpu.max").read().split()
                quota = None if q == "max" else float(q) / float(per)
            except Exception:
                pass
            counts = sorted({c for c in (usable, max(1, usable // 2), max(1, usable // 4), int(quota) if quota else 0) if c >= 1})
            best, timing = None, {}
            probe = min(args.records, 5000)              # large enough that thread start-up does not decide
            for c in counts:
                oracle.set_num_threads(c)
                cpu_run(probe)
                timing[c] = min(cpu_run(probe)[0] for _ in range(2))
                if best is None or timing[c] < timing[best]:
                    best = c
            oracle.set_num_threads(best)
            dt = timing[best]
            nrec = int(max(probe, min(args.records, probe * args.cpu_seconds / max(dt, 1e-6))))
            dt, ref_seq, ref_st = cpu_run(nrec)
            nwin = nrec * (args.length - args.width + 1)
            result["cpu_baseline"] = {
                "value": nwin / dt, "unit": "windows/s", "cores": oracle.num_threads(), "kind": "port",
                "sample": "first %d of %d records (%d windows), oracle/pfm_oracle.c stream_seq + stream_struct_f32, "
                          "OpenMP over positions, %.2f s" % (nrec, args.records, nwin, dt),
                "host_cpus": os.cpu_count(), "usable_cpus": usable, "cgroup_cpu_quota": quota,
                "cores_note": "threads = the fastest of %s on a %d-record probe (seconds: %s); the process may run on %d of the "
                              "host's %d logical CPUs, cgroup cpu.max allows %s CPUs' worth of time"
                              % (counts, probe, {k: round(v, 3) for k, v in timing.items()}, usable, os.cpu_count(), quota),
            }
            got_seq = out_seq[: nrec * stride].cpu().numpy()
            got_st = out_st[: nrec * stride].cpu().numpy()
            nan_ok = bool(np.array_equal(np.isnan(got_seq), np.isnan(ref_seq)))
            v = ~np.isnan(ref_seq)
            seq_ok = nan_ok and bool(np.array_equal(got_seq[v].view(np.uint32), ref_seq[v].view(np.uint32)))
            vs = np.isfinite(ref_st) & (np.abs(ref_st) < 1e9)
            st_err = float(np.abs(got_st[vs] - ref_st[vs]).max())
            big = ~vs & ~np.isnan(ref_st)
            big_ok = bool(np.array_equal(np.isnan(got_st), np.isnan(ref_st)) and
                          np.allclose(got_st[big], ref_st[big], rtol=1e-12, atol=0, equal_nan=True))
            result["parity_on_sample"] = {"oracle_input": "same float32 profile (the synthetic stream is born float32: this measures the "
                                                          "arithmetic, not what float32 STORAGE costs against float64 inputs -- that is "
                                                          "bounded per PFM by scanner.float32_storage_bound and measured on the reference's "
                                                          "example in tests/test_gpu_parity.py)",
                                          "seq_f32_bit_exact": seq_ok, "struct_max_abs_err": st_err,
                                          "struct_within_1e-6": bool(st_err <= 1e-6 and big_ok)}
            result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
            if not args.no_ref_structured:
                # B-ref: the reference's own cost structure (per-window Python loop + C call,
                # pandas iloc + np.dot + nan_to_num, multiprocessing.Pool over records) on a
                # small sample of the same records, scaled linearly in records (independent)
                from oracle import ref_structured
                cores = min(best, 128)           # worker processes: the thread count chosen above (pandas workers beyond 128 only thrash)
                n_seq, n_st = cores * 4, cores
                lut = np.array(list("ACGU") + ["N"] * 4)
                seqs, profs = [], []
                for r in range(n_seq):
                    c = codes[r * stride: r * stride + args.length].cpu().numpy()
                    seqs.append("".join(lut[c]))
                for r in range(n_st):
                    profs.append(profile[r * stride: r * stride + args.length].cpu().numpy().astype(np.float64))
                t_seq, t_st, _, _ = ref_structured.time_reference_structured(seqs, profs, table[:, :4].copy(), spssm, 6.0, cores)
                per_rec = t_seq / n_seq + t_st / n_st          # wall seconds per record with `cores` workers
                wpr = args.length - args.width + 1
                result["cpu_baseline_reference_structured"] = {
                    "value": wpr / per_rec, "unit": "windows/s", "cores": cores, "kind": "port",
                    "sample": "reference cost model (oracle/ref_structured.py): Pool(%d); sequence side %d records in %.2f s, "
                              "averaged-structure side %d records in %.2f s, scaled linearly in records"
                              % (cores, n_seq, t_seq, n_st, t_st),
                }
                result["speedup_vs_reference_structured"] = result["value"] / (wpr / per_rec)
        if (args.full and dist is None and not args.no_secondary and args.workload == "c3" and args.mode == "scores" and not args.from_host
                and args.profile_dtype == "float32"):
            # last: the legs reuse (and overwrite) the headline's output arrays, whose parity sample has been checked above
            result["secondary"] = secondary_legs(torch, _lib, ctx, args, dev, codes, profile, ptype, n_pos, out_seq, out_st,
                                                 stream, windows)
        print(json.dumps(result))
        sys.stdout.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
