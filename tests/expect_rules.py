"""A numpy restatement of the expected counts (include/pfmscan.h "expected counts", DESIGN.md 5h;
rnascan_amd/csrc/pfmscan_expect.hip), built on the occupancy's rules (tests/occupancy_rules.py): the term of a window and the
left-aligned tree of fan-in 32 are taken from there, the weight of a window and the selection by letter are stated here.  No
tolerance in any of it: the GPU tests compare bit patterns.

The two bounds at the end tie the matrix to the occupancy; they are derived here, not tuned.
"""
from fractions import Fraction

import numpy as np

import occupancy_rules as orules
from occupancy_rules import FANIN, U, same_bits, tree_bound  # noqa: F401  (the tests take them from here)

RATIO, POSTERIOR = 0, 1


# ---- the definitions -------------------------------------------------------------------------------------------------
def weights(t, has, occ, mode):
    """w_s of every window: the term (RATIO), or the term times v = 1.0 / occ -- one rounded division per record and motif,
    one rounded product per window (POSTERIOR); occ == +0.0: every weight +0.0.  Windows without a term: +0.0."""
    t = np.asarray(t, dtype=np.float64)
    if mode == RATIO:
        return np.where(has, t, 0.0)
    occ = np.float64(occ)
    if occ == 0.0:
        return np.zeros(t.size)
    with np.errstate(all="ignore"):
        v = np.float64(1.0) / occ
        return np.where(has, t * v, 0.0)


def tree_rows(X):
    """occupancy_rules.tree over every row of X [cells][n_win] at once -> float64 [cells]"""
    a = np.asarray(X, dtype=np.float64)
    if a.shape[1] == 0:
        return np.zeros(a.shape[0])
    with np.errstate(all="ignore"):
        while a.shape[1] > 1:
            pad = (-a.shape[1]) % FANIN
            if pad:
                a = np.concatenate([a, np.zeros((a.shape[0], pad))], axis=1)
            a = a.reshape(a.shape[0], -1, FANIN)
            s = a[:, :, 0]
            for i in range(1, FANIN):
                s = s + a[:, :, i]
            a = s
    return a[:, 0].copy()


def expected_record(codes, off, length, R, n_letters, mode):
    """one record under one motif -> (E float64 [m][8], occ, windows with a term)"""
    R = np.asarray(R, dtype=np.float64)
    m = R.shape[0]
    t, has = orules.terms(codes, off, length, R, n_letters)
    occ = orules.tree(t)
    E = np.zeros((m, 8))
    n_win = t.size
    if n_win == 0:
        return E, occ, 0
    w = weights(t, has, occ, mode)
    c = np.asarray(codes[int(off):int(off) + int(length)]) & 7
    X = np.zeros((m * n_letters, n_win))
    for k in range(m):
        ck = c[k:k + n_win]
        for l in range(n_letters):
            X[k * n_letters + l] = np.where(has & (ck == l), w, 0.0)
    E[:, :n_letters] = tree_rows(X).reshape(m, n_letters)
    return E, occ, int(has.sum())


def expected(codes, offsets, lengths, tables, n_letters, mode):
    """-> exp float64 [n_rec][n_motifs][m][8], occ float64 [n_rec][n_motifs], windows int64 [n_rec]; tables [n_motifs][m][8]"""
    tables = np.asarray(tables, dtype=np.float64)
    if tables.ndim == 2:
        tables = tables[None]
    n_rec, n_q, m = len(offsets), tables.shape[0], tables.shape[1]
    exp = np.zeros((n_rec, n_q, m, 8))
    occ = np.zeros((n_rec, n_q))
    win = np.zeros(n_rec, dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(n_q):
            exp[r, q], occ[r, q], win[r] = expected_record(codes, o, n, tables[q], n_letters, mode)
    return exp, occ, win


def column_sums(E, n_letters):
    """the exact sum over the letters of every motif column, as fractions (finite cells)"""
    return [sum((Fraction(float(x)) for x in row[:n_letters]), Fraction(0)) for row in np.asarray(E, dtype=np.float64)]


# ---- bounds ----------------------------------------------------------------------------------------------------------
def ratio_column_bound(n_win):
    """RATIO mode, finite terms: |sum_c E[k][c] - occ| <= ratio_column_bound(n_win) * occ for every k, the sum over c exact.

    A window with a term adds its term t_s to exactly one letter of column k and +0.0 to the others, so the EXACT sums of
    the n_letters cells add up to T = the exact sum of the record's terms.  Every cell is a tree over non-negative values
    and so within tree_bound(n_win) relative of its exact sum: the exact sum of the computed cells is within tree_bound of T.
    The occupancy is the same tree over all terms: within tree_bound of T as well.  Together 2 * tree_bound * T, and T is occ
    to first order in U, the order to which tree_bound itself is stated (what is dropped is below 1e-13 of the bound).  A
    lone window (depth 0) is copied, not added: the bound is 0."""
    return 2.0 * tree_bound(n_win)


def posterior_column_bound(n_win):
    """POSTERIOR mode, occ finite and > 0, weights that stay normal: |sum_c E[k][c] - 1| <= posterior_column_bound(n_win)
    for every k, the sum over c exact.

    occ = T (1 + a), |a| <= tree_bound; v = (1 / occ)(1 + b), |b| <= U (one rounded division); w_s = t_s v (1 + d_s),
    |d_s| <= U (one rounded product); the cells of a column partition the weights as above and each is a tree over its
    share, within tree_bound relative.  So sum_c E[k][c] = (T / occ)(1 + b)(1 + d)(1 + e) with |e| <= tree_bound, which is
    1 - a + b + d + e to first order: 2 * tree_bound + 2 U."""
    return 2.0 * tree_bound(n_win) + 2.0 * U
