"""A numpy restatement of the expected counts on averaged-structure profiles (include/pfmscan.h "expected counts on
averaged-structure profiles"; rnascan_amd/csrc/pfmscan_expect_profile.hip).  Nothing is derived again: the
term of a window is occupancy_profile_rules.terms (structure only, joint) or occupancy_rules.terms (sequence only), the
weight is expect_rules.weights, the sum is expect_rules.tree_rows.  What is stated here is the value that is summed:
``w_s * r[s + k][c]``, one rounded product (numpy multiplies whole arrays: nothing is fused), +0.0 for a window without a
term.  No tolerance in any of it: the GPU tests compare bit patterns.
"""
import numpy as np

import expect_rules as erules
import occupancy_profile_rules as prules
import occupancy_rules as orules
from expect_rules import POSTERIOR, RATIO  # noqa: F401  (the tests take them from here)
from occupancy_rules import same_bits  # noqa: F401

NSTRUCT = prules.NSTRUCT


def product(w, x):
    """the value of a window with a term under one (column, letter): one rounded product of doubles"""
    return w * x


def expected_record(profile, off, length, S=None, codes=None, R=None, mode=POSTERIOR, prod=None, weights=None, tree_rows=None):
    """one record under one motif -> (exp_struct float64 [m][8], exp_seq float64 [m][8] | None, occ, windows with a term).
    S [m][7] in the profile's stored column order and / or R [m][8] over the 4 RNA letters choose the weight.  ``prod``,
    ``weights``, ``tree_rows``: others in their places (the CPU tests put deliberate mistakes there)"""
    prod, weights, tree_rows = prod or product, weights or erules.weights, tree_rows or erules.tree_rows
    if S is None and R is None:
        raise ValueError("S and R are both None")
    if S is not None:
        t, has = prules.terms(profile, off, length, S, codes, R)
        m = np.asarray(S).shape[0]
    else:
        t, has = orules.terms(codes, off, length, np.asarray(R, dtype=np.float64), 4)
        m = np.asarray(R).shape[0]
    occ = orules.tree(t)
    Es = np.zeros((m, 8))
    Eq = None if R is None else np.zeros((m, 8))
    n_win = t.size
    if n_win == 0:
        return Es, Eq, occ, 0
    w = weights(t, has, occ, mode)
    x = np.asarray(profile[int(off):int(off) + int(length)]).astype(np.float64)       # float rows widened first (exact)
    X = np.zeros((m * NSTRUCT, n_win))
    with np.errstate(all="ignore"):
        for k in range(m):
            for c in range(NSTRUCT):
                X[k * NSTRUCT + c] = np.where(has, prod(w, x[k:k + n_win, c]), 0.0)
    Es[:, :NSTRUCT] = tree_rows(X).reshape(m, NSTRUCT)
    if R is not None:
        cd = np.asarray(codes[int(off):int(off) + int(length)]) & 7
        Y = np.zeros((m * 4, n_win))
        for k in range(m):
            ck = cd[k:k + n_win]
            for l in range(4):
                Y[k * 4 + l] = np.where(has & (ck == l), w, 0.0)
        Eq[:, :4] = erules.tree_rows(Y).reshape(m, 4)
    return Es, Eq, occ, int(has.sum())


def _stack(tables):
    if tables is None:
        return None
    t = np.asarray(tables, dtype=np.float64)
    return t[None] if t.ndim == 2 else t


def expected(profile, offsets, lengths, struct_tables=None, codes=None, seq_tables=None, mode=POSTERIOR, **wrong):
    """-> exp_struct float64 [n_rec][n_motifs][m][8], exp_seq the same | None, occ float64 [n_rec][n_motifs], windows int64
    [n_rec]; struct_tables [n_motifs][m][7] | None, seq_tables [n_motifs][m][8] | None"""
    st, sq = _stack(struct_tables), _stack(seq_tables)
    n_q, m = (st if st is not None else sq).shape[:2]
    n_rec = len(offsets)
    Es = np.zeros((n_rec, n_q, m, 8))
    Eq = None if sq is None else np.zeros((n_rec, n_q, m, 8))
    occ = np.zeros((n_rec, n_q))
    win = np.zeros(n_rec, dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(n_q):
            es, eq, occ[r, q], win[r] = expected_record(profile, o, n, None if st is None else st[q], codes, None if sq is None else sq[q], mode,
                                                        **wrong)
            Es[r, q] = es
            if eq is not None:
                Eq[r, q] = eq
    return Es, Eq, occ, win


def same(got, want):
    """every output of a call: bit patterns (NaN == NaN), exp_seq None on both sides or on neither, Windows equal"""
    if (got[1] is None) != (want[1] is None):
        return False
    return bool(same_bits(got[0], want[0]) and (got[1] is None or same_bits(got[1], want[1])) and same_bits(got[2], want[2]) and
                np.asarray(got[3]).dtype == np.int64 and np.array_equal(got[3], want[3]))
