"""Every branch of hits_core (csrc/pfmscan_api.hip), the two-phase path behind pfmscan_hits_adaptive_dev, pfmscan_hits_staged
and pfmscan_hits_host, on the smallest stream on which its pilot runs and a candidate shard can overflow.

The pilot (a letters pass over the first max(2^22, n / 64) positions) runs when the stream is longer than that; the candidate
budget is max(n / 32, 1024) windows, one of the 32 candidate shards holds min(budget, budget / 32 * 2 + 4096).  The streams
here have 4.9 x 10^6 positions, tiled from a pool of 200 random records:
  stream A   random letters throughout: a selective letter threshold is selective everywhere
  stream B   the same, but behind the pilot's prefix every letter is the one the letter table rewards: the pilot sees a
             selective threshold, the full letters pass overflows every candidate shard
Cases (each in a fresh context, through pfmscan_hits_adaptive_dev -- single-shard sink -- and pfmscan_hits_host -- 32 shards,
sorted): pilot selective and stream selective (k_struct_at); pilot dense (fused pass); pilot selective but stream dense
(overflow, fused pass); selective / dense / selective on ONE context (ctx->two_phase_hot: the dense call arrives hot, skips
the pilot, overflows and falls back; the last call runs the pilot again); the first case with PFMSCAN_TWO_PHASE=0.
The reference is the oracle over the whole stream: hit positions exact, float32 sequence scores bit-exact, structure scores
to their rounding-error bound at the hits.  The tests assert results only; which kernels each case launches is read from a
kernel trace."""
import types

import numpy as np
import pytest

from conftest import assert_f32_bits_equal
from precision_rules import assert_struct_tight
from test_gpu_parity import rand_stream, rand_struct_pssm

pytestmark = pytest.mark.gpu

M = 12
N_TARGET = 4_900_000
PILOT_N = 1 << 22
HIT_SHARDS = 32


@pytest.fixture(scope="module")
def streams(oracle):
    """both streams, their oracle scores and the thresholds, built once and left unchanged"""
    import torch
    from rnascan_amd import pack
    rng = np.random.default_rng(2718)
    pool = rand_stream(rng, 200, 0, 3000)
    pieces_c, pieces_p, n = [], [], 0
    while n < N_TARGET:
        r = int(rng.integers(0, len(pool.offsets)))
        o, L = int(pool.offsets[r]), int(pool.lengths[r]) + 1                 # the record and its separator
        pieces_c.append(pool.codes[o:o + L])
        pieces_p.append(pool.profile[o:o + L])
        n += L
    z = types.SimpleNamespace()
    z.codes_a = np.concatenate(pieces_c)
    z.profile = np.concatenate(pieces_p)
    z.n = n
    assert z.codes_a[-1] == pack.SEP and z.n - PILOT_N >= 700_000
    # a letter table that rewards letter 0; behind the pilot's prefix stream B holds that letter only (separators stay)
    z.T = np.full((M, 8), np.nan)
    z.T[:, :4] = rng.normal(-0.5, 1.5, size=(M, 4))
    z.T[:, 0] = 2.0 + rng.random(M)
    z.P = rand_struct_pssm(rng, M)
    z.codes_b = z.codes_a.copy()
    tail = z.codes_b[PILOT_N:]
    tail[tail != pack.SEP] = 0
    z.seq_a, z.seq_b = oracle.stream_seq(z.codes_a, z.T), oracle.stream_seq(z.codes_b, z.T)
    z.st = oracle.stream_struct(z.profile, z.P)
    fin = z.seq_a[:PILOT_N][np.isfinite(z.seq_a[:PILOT_N])]
    z.thr_selective = float(np.quantile(fin, 0.995))
    z.thr_dense = float(np.quantile(fin, 0.5))
    fst = z.st[np.isfinite(z.st)]
    z.thr_st = {"selective": float(np.quantile(fst, 0.8)), "dense": float(np.quantile(fst, 0.998)), "overflow": float(np.quantile(fst, 0.99))}
    # the construction reaches its branches (hits_core's own arithmetic, on the oracle's scores)
    budget = max(z.n // 32, 1024)
    shard_cap = min(budget, budget // HIT_SHARDS * 2 + 4096)
    assert PILOT_N == max(1 << 22, z.n // 64) and PILOT_N < z.n                                   # the pilot runs
    for seq in (z.seq_a, z.seq_b):
        assert int((seq[:PILOT_N] > z.thr_selective).sum()) * 32 < PILOT_N                        # ... and finds the threshold selective
    assert int((z.seq_a[:PILOT_N] > z.thr_dense).sum()) * 32 > 2 * PILOT_N                        # ... or dense
    n_cand_a = int((z.seq_a > z.thr_selective).sum())
    assert n_cand_a * 4 < budget and n_cand_a < shard_cap * 4                                     # A: no overflow, and the context turns hot
    assert int((z.seq_b[PILOT_N:] > z.thr_selective).sum()) > 32 * shard_cap                      # B: every candidate shard overflows
    dev = torch.device("cuda:0")
    z.d_codes = {"A": torch.from_numpy(z.codes_a).to(dev), "B": torch.from_numpy(z.codes_b).to(dev)}
    z.d_profile = torch.from_numpy(z.profile).to(dev)
    z.want = {}
    return z


def _want(oracle, z, which, thr_seq, thr_st):
    key = (which, thr_seq, thr_st)
    if key not in z.want:
        z.want[key] = oracle.stream_hits(z.seq_a if which == "A" else z.seq_b, z.st, thr_seq, thr_st)
    return z.want[key]


def _check(oracle, z, which, thr_seq, thr_st, pos, sq, st):
    want = _want(oracle, z, which, thr_seq, thr_st)
    assert 1000 < len(want) < 20000
    assert np.array_equal(pos, want), (len(pos), len(want))
    assert_f32_bits_equal(sq, (z.seq_a if which == "A" else z.seq_b)[want])
    assert_struct_tight(st, z.profile, z.P, positions=want)


CALLS = {                                                 # case -> [(stream, letter threshold, structure threshold)]
    "pilot_selective_stream_selective": [("A", "selective", "selective")],
    "pilot_dense": [("A", "dense", "dense")],
    "pilot_selective_stream_dense": [("B", "selective", "overflow")],
    "hot_sequence": [("A", "selective", "selective"), ("B", "selective", "overflow"), ("A", "selective", "selective")],
    "two_phase_off": [("A", "selective", "selective")],
}


@pytest.mark.parametrize("case", list(CALLS))
def test_hits_core_branch(case, streams, oracle, monkeypatch):
    from rnascan_amd import _lib
    z = streams
    if case == "two_phase_off":
        monkeypatch.setenv("PFMSCAN_TWO_PHASE", "0")
    # one context per entry-point form: ctx->two_phase_hot is driven by one form's calls alone
    for form in ("dev", "host"):
        with _lib.Context(0) as c:
            motif = c.motif(z.T, z.P)
            for which, seq_kind, st_kind in CALLS[case]:
                thr_seq = z.thr_selective if seq_kind == "selective" else z.thr_dense
                _one_form(form, c, motif, oracle, z, which, thr_seq, z.thr_st[st_kind])
            motif.close()


def _one_form(form, c, motif, oracle, z, which, thr_seq, thr_st):
    import torch
    from rnascan_amd import _lib
    if form == "host":
        pos, sq, st = c.hits_host(motif, z.codes_a if which == "A" else z.codes_b, z.profile, thr_seq, thr_st, capacity=1 << 17)
        _check(oracle, z, which, thr_seq, thr_st, pos, sq, st)
        return
    cap = 1 << 15
    dev = torch.device("cuda:0")
    d_pos = torch.empty(cap, dtype=torch.int64, device=dev)
    d_sq = torch.empty(cap, dtype=torch.float32, device=dev)
    d_st = torch.empty(cap, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    c.hits_adaptive_dev(motif, z.d_codes[which].data_ptr(), z.d_profile.data_ptr(), _lib.PROFILE_F32, z.n, thr_seq, thr_st, cap,
                        d_pos.data_ptr(), d_sq.data_ptr(), d_st.data_ptr(), d_cnt.data_ptr())
    c.synchronize()
    k = int(d_cnt.item())
    assert k <= cap
    pos = d_pos[:k].cpu().numpy()
    order = np.argsort(pos, kind="stable")
    _check(oracle, z, which, thr_seq, thr_st, pos[order], d_sq[:k].cpu().numpy()[order], d_st[:k].cpu().numpy()[order])
