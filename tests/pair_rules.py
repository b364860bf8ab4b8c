"""A numpy restatement of the occupancy and the expected counts of two code streams (include/pfmscan.h "occupancy and expected
counts of two code streams"), built on the single-stream rules (tests/occupancy_rules.py, tests/expect_rules.py):
the tree, the weight of a window and the bit comparison are taken from there; the joint term, which windows have one and the
selection by the letter of either stream are stated here.  No tolerance in any of it: the GPU tests compare bit patterns.
"""
import numpy as np

import expect_rules as erules
import occupancy_rules as orules
from occupancy_rules import same_bits, stream, table  # noqa: F401  (the tests take them from here)

RATIO, POSTERIOR = erules.RATIO, erules.POSTERIOR
N_SEQ, N_STRUCT = 4, 7
LDS_DOUBLES = 2048     # OCC_LDS_DOUBLES of csrc/pfmscan_occupancy.hip: table cells of one chunk, padding included
PAIR_LETTERS = 11      # OCC_PAIR_LETTERS: the 4 + 7 letters of a row of a pair's tables in LDS


def terms(codes, codes2, off, length, R, S):
    """the record's windows in order -> (t float64 [n_win] with +0.0 where the window has no term, has bool [n_win]):
    t = R[0][a_0], t = t * R[k][a_k] for k = 1 .. m-1, then t = t * S[k][b_k] for k = 0 .. m-1 -- whole arrays, one rounded
    product per window and step; has: every a_k < 4 and every b_k < 7"""
    R, S = np.asarray(R, dtype=np.float64), np.asarray(S, dtype=np.float64)
    m = R.shape[0]
    assert S.shape == R.shape
    n_win = max(int(length) - m + 1, 0)
    if n_win == 0:
        return np.zeros(0), np.zeros(0, dtype=bool)
    a = np.asarray(codes[int(off):int(off) + int(length)]) & 7
    b = np.asarray(codes2[int(off):int(off) + int(length)]) & 7
    with np.errstate(all="ignore"):
        t = R[0][a[0:n_win]]
        for k in range(1, m):
            t = t * R[k][a[k:k + n_win]]
        for k in range(m):
            t = t * S[k][b[k:k + n_win]]
    has = np.ones(n_win, dtype=bool)
    for k in range(m):
        has &= (a[k:k + n_win] < N_SEQ) & (b[k:k + n_win] < N_STRUCT)
    return np.where(has, t, 0.0), has


def _stack(T):
    T = np.asarray(T, dtype=np.float64)
    return T[None] if T.ndim == 2 else T


def occupancy(codes, codes2, offsets, lengths, seq_tables, struct_tables):
    """-> occ float64 [n_rec][n_pairs], windows int64 [n_rec]; both table arrays [n_pairs][m][8]"""
    Rs, Ss = _stack(seq_tables), _stack(struct_tables)
    occ = np.zeros((len(offsets), Rs.shape[0]))
    win = np.zeros(len(offsets), dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(Rs.shape[0]):
            t, has = terms(codes, codes2, o, n, Rs[q], Ss[q])
            occ[r, q] = orules.tree(t)
            win[r] = int(has.sum())
    return occ, win


def expected_record(codes, codes2, off, length, R, S, mode):
    """one record under one pair -> (E_seq float64 [m][8], E_struct float64 [m][8], occ, windows with a term)"""
    m = np.asarray(R).shape[0]
    t, has = terms(codes, codes2, off, length, R, S)
    occ = orules.tree(t)
    Es, Et = np.zeros((m, 8)), np.zeros((m, 8))
    n_win = t.size
    if n_win == 0:
        return Es, Et, occ, 0
    w = erules.weights(t, has, occ, mode)
    a = np.asarray(codes[int(off):int(off) + int(length)]) & 7
    b = np.asarray(codes2[int(off):int(off) + int(length)]) & 7
    X = np.zeros((m * (N_SEQ + N_STRUCT), n_win))
    for k in range(m):
        ak, bk = a[k:k + n_win], b[k:k + n_win]
        for c in range(N_SEQ):
            X[k * N_SEQ + c] = np.where(has & (ak == c), w, 0.0)
        for c in range(N_STRUCT):
            X[m * N_SEQ + k * N_STRUCT + c] = np.where(has & (bk == c), w, 0.0)
    sums = erules.tree_rows(X)
    Es[:, :N_SEQ] = sums[:m * N_SEQ].reshape(m, N_SEQ)
    Et[:, :N_STRUCT] = sums[m * N_SEQ:].reshape(m, N_STRUCT)
    return Es, Et, occ, int(has.sum())


def expected(codes, codes2, offsets, lengths, seq_tables, struct_tables, mode):
    """-> exp_seq, exp_struct float64 [n_rec][n_pairs][m][8], occ float64 [n_rec][n_pairs], windows int64 [n_rec]"""
    Rs, Ss = _stack(seq_tables), _stack(struct_tables)
    n_rec, n_q, m = len(offsets), Rs.shape[0], Rs.shape[1]
    es, et = np.zeros((n_rec, n_q, m, 8)), np.zeros((n_rec, n_q, m, 8))
    occ = np.zeros((n_rec, n_q))
    win = np.zeros(n_rec, dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(n_q):
            es[r, q], et[r, q], occ[r, q], win[r] = expected_record(codes, codes2, o, n, Rs[q], Ss[q], mode)
    return es, et, occ, win


def ones(m):
    """the table whose every cell is 1.0: multiplying by it is exact"""
    return np.ones((m, 8))


def lds_chunk(m, n_q=1 << 20):
    """pairs per LDS chunk of k_occ_blocks<QN, true> (the chunk rule stated above it in csrc/pfmscan_occupancy.hip): the most
    c <= n_q with m * 11 * ls(c) <= LDS_DOUBLES, at least 1"""
    def ls(nq):
        qn = 8 if nq >= 8 else 4 if nq >= 4 else 2 if nq >= 2 else 1
        x = -(-nq // qn) * qn
        return x + 2 if x % 16 == 0 else x
    c = max(1, min(n_q, LDS_DOUBLES // (m * PAIR_LETTERS)))
    while c > 1 and m * PAIR_LETTERS * ls(c) > LDS_DOUBLES:
        c -= 1
    return c


def streams(rng, lengths, foreign_seq=0.0, foreign_struct=0.0, case=False):
    """two streams over one record table -> (codes, codes2, offsets, lengths)"""
    codes, off, lens = orules.stream(rng, lengths, N_SEQ, foreign=foreign_seq)
    codes2, _, _ = orules.stream(rng, lengths, N_STRUCT, foreign=foreign_struct, case=case)
    return codes, codes2, off, lens
