"""A numpy restatement of the expected letter-PAIR table of two code streams (include/pfmscan.h "The expected letter-PAIR table
per column"): ``expected_record`` / ``expected`` of tests/pair_rules.py extended by the table.  The joint term and
which windows have one are pair_rules.terms, the weight is expect_rules.weights, the tree expect_rules.tree_rows over 28 m more
rows; only the selection by the letter PAIR is stated here.  No tolerance in any of it: the GPU tests compare bit patterns.
"""
import numpy as np

import expect_rules as erules
import occupancy_rules as orules
import pair_rules as prules
from pair_rules import N_SEQ, N_STRUCT, POSTERIOR, RATIO, lds_chunk, ones, same_bits, streams, table  # noqa: F401  (the tests take them from here)

N_JOINT = N_SEQ * N_STRUCT


def expected_record(codes, codes2, off, length, R, S, mode):
    """one record under one pair -> (E_seq float64 [m][8], E_struct float64 [m][8], E_joint float64 [m][4][8], occ, windows with
    a term); E_joint[k][a][b] is the tree sum of (has_s && a_k == a && b_k == b) ? w_s : +0.0, column b = 7 is +0.0"""
    m = np.asarray(R).shape[0]
    t, has = prules.terms(codes, codes2, off, length, R, S)
    occ = orules.tree(t)
    Es, Et, Ej = np.zeros((m, 8)), np.zeros((m, 8)), np.zeros((m, N_SEQ, 8))
    n_win = t.size
    if n_win == 0:
        return Es, Et, Ej, occ, 0
    w = erules.weights(t, has, occ, mode)
    a = np.asarray(codes[int(off):int(off) + int(length)]) & 7
    b = np.asarray(codes2[int(off):int(off) + int(length)]) & 7
    X = np.zeros((m * (N_SEQ + N_STRUCT + N_JOINT), n_win))
    j0 = m * (N_SEQ + N_STRUCT)
    for k in range(m):
        ak, bk = a[k:k + n_win], b[k:k + n_win]
        for c in range(N_SEQ):
            X[k * N_SEQ + c] = np.where(has & (ak == c), w, 0.0)
        for c in range(N_STRUCT):
            X[m * N_SEQ + k * N_STRUCT + c] = np.where(has & (bk == c), w, 0.0)
        for ca in range(N_SEQ):
            for cb in range(N_STRUCT):
                X[j0 + (k * N_SEQ + ca) * N_STRUCT + cb] = np.where(has & (ak == ca) & (bk == cb), w, 0.0)
    sums = erules.tree_rows(X)
    Es[:, :N_SEQ] = sums[:m * N_SEQ].reshape(m, N_SEQ)
    Et[:, :N_STRUCT] = sums[m * N_SEQ:j0].reshape(m, N_STRUCT)
    Ej[:, :, :N_STRUCT] = sums[j0:].reshape(m, N_SEQ, N_STRUCT)
    return Es, Et, Ej, occ, int(has.sum())


def expected(codes, codes2, offsets, lengths, seq_tables, struct_tables, mode):
    """-> exp_seq, exp_struct float64 [n_rec][n_pairs][m][8], exp_joint float64 [n_rec][n_pairs][m][4][8], occ float64
    [n_rec][n_pairs], windows int64 [n_rec]"""
    Rs, Ss = prules._stack(seq_tables), prules._stack(struct_tables)
    n_rec, n_q, m = len(offsets), Rs.shape[0], Rs.shape[1]
    es, et, ej = np.zeros((n_rec, n_q, m, 8)), np.zeros((n_rec, n_q, m, 8)), np.zeros((n_rec, n_q, m, N_SEQ, 8))
    occ = np.zeros((n_rec, n_q))
    win = np.zeros(n_rec, dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(n_q):
            es[r, q], et[r, q], ej[r, q], occ[r, q], win[r] = expected_record(codes, codes2, o, n, Rs[q], Ss[q], mode)
    return es, et, ej, occ, win


def pair_counts(codes, codes2, offsets, lengths, m):
    """the integer count of letter pairs under every window of every record, int64 [m][8][8] by code (7: foreign): what
    pfmscan_site_joint_* counts when every window start is a hit (flank 0)"""
    J = np.zeros((m, 8, 8), dtype=np.int64)
    for o, n in zip(offsets, lengths):
        n_win = max(int(n) - m + 1, 0)
        a = np.asarray(codes[int(o):int(o) + int(n)]).astype(np.int64) & 7
        b = np.asarray(codes2[int(o):int(o) + int(n)]).astype(np.int64) & 7
        for k in range(m):
            np.add.at(J[k], (a[k:k + n_win], b[k:k + n_win]), 1)
    return J
