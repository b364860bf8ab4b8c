"""The MID-TILE flush of the wave-private hit queues (csrc/pfmscan_hitqueue.hpp: WaveHitQueue::ensure_room) on the credit
kernels, which no uniform stream reaches: at a threshold selective enough for the credit table's predicted survivor rate to
keep the launch on k_letters_cred / k_letters_cred8, a wave of random letters parks at most a few dozen hits per tile.

The stream here is ~3 tiles of 4096 positions of random letters with ONE planted homopolymer run of 2500 positions across
the first tile boundary; the tables give the run's letter the row maximum in every row and the threshold lies just below the
run's score.  Every window of the run is a hit -- 1024 in the waves the run covers, against queues of 256 (k_letters_cred),
128 (its two-stream form) and 128 (k_letters_cred8) -- while a window of uniform letters survives the prefilter with
probability ~4^-m.  A workgroup walks three tiles (PFMSCAN_TILES_PER_BLOCK=3, fresh Context), so the queue also lives
across the tile boundary inside the run.  The library pair scores the same stream with nine motifs of which one is the
planted table: phase B of k_library / k_library8 sees full 64-hit ballots (the run, motif 0) next to empty ones.

Against the oracle: positions exact, float32 scores bit for bit, fp64 scores equal.  The tests assert results only.  Which
kernels ran was confirmed once with a kernel trace of this file: k_letters_cred<3, false>, k_letters_cred<3, true>,
k_letters_cred8<6>, k_library<2, 8, float, false> and k_library8<2, 16>.  The assertions on the credit tables
(_stays_on_credit_kernel, credit8_table) only keep a later change of tables or thresholds from leaving those kernels
unnoticed; they restate the launcher's 1/32 rule and would have to follow it."""
import types

import numpy as np
import pytest

from conftest import assert_f32_bits_equal
from test_gpu_letters8 import _between, _table
from test_gpu_library import oracle_library_hits
from test_gpu_parity import rand_table

pytestmark = pytest.mark.gpu

N = 12800                                                 # 3 tiles of 4096 and a ragged fourth: two workgroups at 3 tiles each
RUN0, RUN_LEN = 3000, 2500                                # the run covers the last wave of tile 0 and the first of tile 1
LETTER, LETTER2 = 2, 5                                    # the planted letter of the first / second stream


def _plant(T, letter, n_letters):
    """the planted letter gets the row maximum in every row, a clear 1.0 above the next letter: a window with one other
    letter scores at least 1.0 below the run's windows"""
    T = T.copy()
    others = np.delete(T[:, :n_letters], letter, axis=1)
    T[:, letter] = np.nanmax(np.where(np.isfinite(others), others, -np.inf), axis=1) + 1.0 + np.arange(T.shape[0]) * 0.03125
    return T


def _streams():
    from rnascan_amd import pack
    rng = np.random.default_rng(1618)
    z = types.SimpleNamespace()
    c1 = rng.integers(0, 4, size=N).astype(np.uint8)
    c2 = rng.integers(0, 7, size=N).astype(np.uint8)
    foreign = rng.random(N) < 0.002
    foreign[RUN0:RUN0 + RUN_LEN] = False
    c1[foreign] = pack.SEP
    c2[foreign] = pack.SEP
    c1[RUN0:RUN0 + RUN_LEN] = LETTER
    c2[RUN0:RUN0 + RUN_LEN] = LETTER2
    z.s1, z.s2 = pack.pack([c1]), pack.pack([c2])
    assert z.s1.codes.size == z.s2.codes.size and RUN0 < 4096 < RUN0 + RUN_LEN
    return z


@pytest.fixture(scope="module")
def planted():
    """both code streams (4 letters / 7 letters, separators at the same places), built once and left unchanged"""
    return _streams()


@pytest.fixture()
def walk3(monkeypatch):
    from rnascan_amd import _lib
    monkeypatch.setenv("PFMSCAN_TILES_PER_BLOCK", "3")
    with _lib.Context(0) as c:
        yield c


def _just_below_run(scores, m):
    """a threshold below the score of the run's windows and above every other window's"""
    run = np.asarray(scores[RUN0:RUN0 + RUN_LEN - m + 1], dtype=np.float64)
    assert np.all(run == run[0])
    thr = float(run[0]) - 0.5
    n_hits = int((np.asarray(scores, dtype=np.float64) > thr).sum())
    assert RUN_LEN - m + 1 <= n_hits < RUN_LEN + 50, n_hits       # the run, and next to nothing else: a selective threshold
    return thr


def _stays_on_credit_kernel(T, thr):
    """launch_letters_cred's own prediction (csrc/pfmscan_kernels.hip): the share of uniformly drawn windows whose 16-bit
    credit sum reaches the flag bit must not exceed 1/32, or the launch goes to k_letters_pre"""
    from rnascan_amd import _lib
    cr, slack = _lib.credit_table(T, thr)
    dist = {0: 1.0}
    for row in cr:
        nxt = {}
        for v, p in dist.items():
            for c in row:
                w = min(65535, v + int(c))
                nxt[w] = nxt.get(w, 0.0) + p / len(row)
        dist = nxt
    return np.isfinite(slack) and sum(p for v, p in dist.items() if v >= 32768) <= 1.0 / 32.0


def test_letters_run_overflows_the_wave_queue(walk3, planted, oracle):
    """k_letters_cred<3, false>: 1024 hits in a wave against WQ_CAP = 256"""
    m = 10
    rng = np.random.default_rng(1)
    T = _plant(rand_table(rng, m), LETTER, 4)
    want_seq = oracle.stream_seq(planted.s1.codes, T)
    thr = _just_below_run(want_seq, m)
    assert _stays_on_credit_kernel(T, thr)
    motif = walk3.motif(letter_table=T)
    pos, sq, _ = walk3.hits_host(motif, planted.s1.codes, thr_seq=thr)
    want = oracle.stream_hits(want_seq, None, thr, thr)
    assert np.array_equal(pos, want), (pos.size, want.size)
    assert_f32_bits_equal(sq, want_seq[want])
    motif.close()


def test_pair_run_overflows_the_two_score_queue(walk3, planted, oracle):
    """k_letters_cred<3, true>: both streams planted, 1024 combined hits in a wave against a queue of 128"""
    m = 10
    rng = np.random.default_rng(2)
    T1, T2 = _plant(rand_table(rng, m), LETTER, 4), _plant(_table(rng, m), LETTER2, 7)
    sq = oracle.stream_seq(planted.s1.codes, T1)
    st = oracle.stream_letters_f64(planted.s2.codes, T2)
    t1, t2 = _just_below_run(sq, m), _just_below_run(st, m)
    assert _stays_on_credit_kernel(T1, t1)
    a, b = walk3.motif(T1, None), walk3.motif(T2, None)
    pos, gq, gt = walk3.hits_pair_host(a, b, planted.s1.codes, planted.s2.codes, t1, t2)
    want = oracle.stream_hits(sq, st, t1, t2)
    assert want.size >= RUN_LEN - m + 1
    assert np.array_equal(pos, want), (pos.size, want.size)
    assert_f32_bits_equal(gq, sq[want])
    assert np.array_equal(gt, st[want])
    a.close()
    b.close()


def test_letters_f64_run_overflows_the_wave_queue(walk3, planted, oracle):
    """k_letters_cred8<6>: 1024 fp64 hits in a wave against Q8_CAP = 128"""
    from rnascan_amd import _lib
    m = 12
    rng = np.random.default_rng(3)
    T = _plant(_table(rng, m), LETTER2, 7)
    full = oracle.stream_letters_f64(planted.s2.codes, T)
    thr = _just_below_run(full, m)
    assert _lib.credit8_table(T, thr)[1] == 1               # mode 1: the prefilter kernel, not the exact one
    mo = walk3.motif(T, None)
    pos, sc = walk3.hits_letters_f64_host(mo, planted.s2.codes, thr)
    want = oracle.stream_hits(None, full, -np.inf, thr)
    assert np.array_equal(pos, want), (pos.size, want.size)
    assert np.array_equal(sc, full[want])
    mo.close()


def test_library_pair_full_and_empty_ballots(walk3, planted, oracle):
    """nine motifs over the 4-letter stream, as a sequence library (k_library) and as a structure-letter library (k_library8):
    motif 0 is the planted table (every lane of a phase-B batch inside the run is a hit), the others are selective"""
    m, n = 10, 9
    rng = np.random.default_rng(4)
    s = planted.s1
    # sequence library: float32 scores, float32-cast compare
    LT = np.stack([_plant(rand_table(rng, m), LETTER, 4)] + [rand_table(rng, m) for _ in range(n - 1)])
    ts = np.empty(n)
    for k in range(n):
        sq = oracle.stream_seq(s.codes, LT[k])
        ts[k] = _just_below_run(sq, m) if k == 0 else float(np.quantile(sq[np.isfinite(sq)].astype(np.float64), 0.999)) + 1e-4
    lib = walk3.library(LT, None)
    pos, mo, sq, st = walk3.library_hits_host(lib, s.codes, None, ts)
    wp, wm, wsq, _ = oracle_library_hits(oracle, s, LT, None, ts, None)
    assert st is None and RUN_LEN - m + 1 <= wp.size < 4000
    assert np.array_equal(pos, wp) and np.array_equal(mo, wm), (pos.size, wp.size)
    assert_f32_bits_equal(sq, wsq)
    lib.close()
    # structure-letter library over the same codes (letters 0 .. 3 of its seven): fp64 scores, fp64 compare
    ST = np.stack([_plant(_table(rng, m), LETTER, 7)] + [_table(rng, m) for _ in range(n - 1)])
    full = [oracle.stream_letters_f64(s.codes, ST[k]) for k in range(n)]
    tt = np.array([_just_below_run(full[0], m)] + [_between(full[k], 0.999) for k in range(1, n)])
    lib = walk3.library(None, struct_letters=ST)
    pos, mo, _, st = walk3.library_hits_letters_host(lib, s.codes, None, None, tt)
    total = 0
    for k in range(n):
        sel = mo == k
        want = oracle.stream_hits(None, full[k], -np.inf, float(tt[k]))
        assert np.array_equal(pos[sel], want), (k, int(sel.sum()), want.size)
        assert np.array_equal(st[sel], full[k][want])
        total += want.size
    assert pos.size == total and RUN_LEN - m + 1 <= total < 4000
    lib.close()
