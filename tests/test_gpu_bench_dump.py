"""bench.py --dump-outputs DIR: what the last timed step computed, as float32 / float64 .npy files of at most 64 MB, the same
from run to run (the inputs depend on the arguments alone) and equal to the CPU oracle on those inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, assert_f32_bits_equal, assert_struct_close

pytestmark = pytest.mark.gpu
RECORDS, LENGTH, WIDTH = 3000, 3000, 12
STRIDE = LENGTH + 1
N_WIN = LENGTH - WIDTH + 1


def _bench(outdir, *extra):
    env = dict(os.environ, PFMSCAN_BENCH_NO_FLOOR="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--records", str(RECORDS), "--steps", "3", "--warmup", "1",
                        "--settle", "2", "--no-secondary", "--no-ref-structured", "--no-cpu-baseline",
                        "--dump-outputs", str(outdir)] + list(extra), env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    files = sorted(os.listdir(outdir))
    assert sum(os.path.getsize(os.path.join(outdir, f)) for f in files) <= 64 << 20
    arrays = {f[:-4]: np.load(os.path.join(outdir, f)) for f in files}
    assert all(f.endswith(".npy") for f in files) and all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values())       # only windows inside records: no NaN placeholders
    return res, arrays


def _inputs(records):
    """the records bench.py scanned (rank 0's seed), on the host"""
    import torch
    from bench_legs import make_pssms, make_stream
    codes, profile, _ = make_stream(torch, torch.device("cuda", 0), RECORDS, LENGTH, 20240601)
    sel = torch.from_numpy(records)
    c = codes.view(RECORDS, STRIDE)[sel.to(codes.device)].cpu().numpy().reshape(-1)
    p = profile.view(RECORDS, STRIDE, 7)[sel.to(profile.device)].cpu().numpy().reshape(-1, 7)
    del codes, profile
    torch.cuda.empty_cache()
    return c, p, make_pssms(WIDTH)


@pytest.mark.timeout(900)
def test_bench_dump_outputs_scores(tmp_path, oracle):
    _, one = _bench(tmp_path / "one")
    _, two = _bench(tmp_path / "two")
    assert sorted(one) == ["record_index", "scores_seq", "scores_struct"]
    for name in one:
        assert one[name].dtype == two[name].dtype and one[name].tobytes() == two[name].tobytes(), name
    rec = one["record_index"].astype(np.int64)
    # 3000 records of 12 B per window are more than the budget: a sorted sample of whole records, their windows
    assert 0 < len(rec) < RECORDS and np.all(np.diff(rec) > 0) and rec[-1] < RECORDS
    assert one["scores_seq"].shape == one["scores_struct"].shape == (len(rec), N_WIN)
    some = np.arange(0, len(rec), max(1, len(rec) // 16))
    codes, profile, (table, spssm) = _inputs(rec[some])
    # the oracle scores every position of the sampled records laid end to end; a record's windows are its first N_WIN
    want_seq = oracle.stream_seq(codes, table).reshape(len(some), STRIDE)[:, :N_WIN]
    want_st = oracle.stream_struct(profile, spssm).reshape(len(some), STRIDE)[:, :N_WIN]
    assert_f32_bits_equal(one["scores_seq"][some], want_seq)
    assert_struct_close(one["scores_struct"][some], want_st)


@pytest.mark.timeout(900)
def test_bench_dump_outputs_hits(tmp_path, oracle):
    res, got = _bench(tmp_path / "hits", "--mode", "hits")
    assert sorted(got) == ["hit_count", "hit_pos", "hit_seq", "hit_struct"]
    pos = got["hit_pos"].astype(np.int64)
    assert int(got["hit_count"][0]) == len(pos) == res["config"]["hits_per_step"] > 0
    assert np.all(np.diff(pos) > 0)                     # sorted, every window once
    codes, profile, (table, spssm) = _inputs(np.arange(RECORDS))
    seq, st = oracle.stream_seq(codes, table), oracle.stream_struct(profile, spssm)
    want = oracle.stream_hits(seq, st, res["config"]["minscore_seq"], res["config"]["minscore_struct"])
    assert np.array_equal(pos, want)
    assert_f32_bits_equal(got["hit_seq"], seq[want])
    assert_struct_close(got["hit_struct"], st[want])
