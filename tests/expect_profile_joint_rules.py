"""A numpy restatement of the expected nucleotide x context table on averaged-structure profiles (include/pfmscan.h "The
expected nucleotide x context table per column on averaged-structure profiles"; k_expp_blocks<.., JOINT> of
rnascan_amd/csrc/pfmscan_expect_profile.hip).  Nothing is derived again: the term of a window is occupancy_profile_rules.terms
(joint) or occupancy_rules.terms (sequence only), the weight is expect_rules.weights, the sum is expect_rules.tree_rows, the two
matrices are expect_profile_rules.expected_record.  What is stated here is the value that is summed,
``(has_s && (codes[s + k] & 7) == a) ? w_s * r[s + k][c] : +0.0``: the select and one rounded product (numpy multiplies whole
arrays: nothing is fused).  No tolerance in any of it: the GPU tests compare bit patterns.
"""
from fractions import Fraction

import numpy as np

import expect_profile_rules as xrules
import expect_rules as erules
import occupancy_profile_rules as prules
import occupancy_rules as orules
from expect_rules import POSTERIOR, RATIO  # noqa: F401  (the tests take them from here)
from occupancy_rules import U, same_bits  # noqa: F401

NSTRUCT = prules.NSTRUCT
N_SEQ = 4


def product(w, x):
    """the value of a selected window under one (column, nucleotide, profile column): one rounded product of doubles"""
    return w * x


def select(has, ck, a):
    """the windows that count for nucleotide a under a column whose codes are ck: those with a term whose code is a"""
    return has & (ck == a)


def joint_record(profile, codes, off, length, R, S=None, mode=POSTERIOR, prod=None, sel=None, tree_rows=None):
    """one record under one motif (pair) -> exp_joint float64 [m][4][8]: cell [k][a][c], c < 7 in the profile's stored column
    order; column 7 is +0.0.  R [m][8] is needed (the codes are read); S [m][7] or None chooses the joint or the letter chain.
    ``prod``, ``sel``, ``tree_rows``: others in their places (the CPU tests put deliberate mistakes there)"""
    prod, sel, tree_rows = prod or product, sel or select, tree_rows or erules.tree_rows
    if R is None:
        raise ValueError("the table reads the codes: R is needed")
    m = np.asarray(R).shape[0]
    if S is not None:
        t, has = prules.terms(profile, off, length, S, codes, R)
    else:
        t, has = orules.terms(codes, off, length, np.asarray(R, dtype=np.float64), N_SEQ)
    Ej = np.zeros((m, N_SEQ, 8))
    n_win = t.size
    if n_win == 0:
        return Ej
    occ = orules.tree(t)
    w = erules.weights(t, has, occ, mode)
    x = np.asarray(profile[int(off):int(off) + int(length)]).astype(np.float64)       # float rows widened first (exact)
    cd = np.asarray(codes[int(off):int(off) + int(length)]) & 7
    X = np.zeros((m * N_SEQ * NSTRUCT, n_win))
    with np.errstate(all="ignore"):
        for k in range(m):
            ck = cd[k:k + n_win]
            for a in range(N_SEQ):
                on = sel(has, ck, a)
                for c in range(NSTRUCT):
                    X[(k * N_SEQ + a) * NSTRUCT + c] = np.where(on, prod(w, x[k:k + n_win, c]), 0.0)
    Ej[:, :, :NSTRUCT] = tree_rows(X).reshape(m, N_SEQ, NSTRUCT)
    return Ej


def expected_record(profile, codes, off, length, R, S=None, mode=POSTERIOR, **wrong):
    """-> (exp_struct [m][8], exp_seq [m][8], exp_joint [m][4][8], occ, windows with a term): the first two and the last two are
    expect_profile_rules.expected_record's"""
    es, eq, occ, win = xrules.expected_record(profile, off, length, S, codes, R, mode)
    return es, eq, joint_record(profile, codes, off, length, R, S, mode, **wrong), occ, win


def expected(profile, codes, offsets, lengths, seq_tables, struct_tables=None, mode=POSTERIOR, **wrong):
    """-> exp_struct, exp_seq float64 [n_rec][n_motifs][m][8], exp_joint float64 [n_rec][n_motifs][m][4][8], occ float64
    [n_rec][n_motifs], windows int64 [n_rec]; seq_tables [n_motifs][m][8], struct_tables [n_motifs][m][7] | None"""
    st, sq = xrules._stack(struct_tables), xrules._stack(seq_tables)
    n_q, m = sq.shape[:2]
    n_rec = len(offsets)
    Es, Eq, Ej = np.zeros((n_rec, n_q, m, 8)), np.zeros((n_rec, n_q, m, 8)), np.zeros((n_rec, n_q, m, N_SEQ, 8))
    occ = np.zeros((n_rec, n_q))
    win = np.zeros(n_rec, dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(n_q):
            Es[r, q], Eq[r, q], Ej[r, q], occ[r, q], win[r] = expected_record(profile, codes, o, n, sq[q], None if st is None else st[q], mode,
                                                                              **wrong)
    return Es, Eq, Ej, occ, win


def same(got, want):
    """(exp_struct, exp_seq, exp_joint, occ, windows) of a call: bit patterns (NaN == NaN), None on both sides or on neither"""
    for g, w in zip(got[:4], want[:4]):
        if (g is None) != (w is None) or (g is not None and not same_bits(g, w)):
            return False
    return bool(np.asarray(got[4]).dtype == np.int64 and np.array_equal(got[4], want[4]))


# ---- the margin: the table summed over the nucleotides against exp_struct -------------------------------------------------
def tree_depth(n_win):
    """levels of the tree over n_win values (a lone window: 0)"""
    d, n = 0, int(n_win)
    while n > 1:
        n = (n + erules.FANIN - 1) // erules.FANIN
        d += 1
    return d


def margin_bound(n_win, abs_sum):
    """|sum_a exp_joint[k][a][c] - exp_struct[k][c]| <= margin_bound(n_win, A), the sum over a exact, A = the exact sum of |x_s| over
    the windows with a term, x_s = fl(w_s * r[s + k][c]) the value exp_struct sums (finite values).

    A window with a term and a known code adds the SAME rounded product x_s to exp_struct[k][c] and to exactly one of the four
    cells exp_joint[k][a][c], and +0.0 to the other three (has_s implies a known code wherever R is given).  So the exact sums of
    the four cells' values add up to X = the exact sum of the x_s, the exact sum of exp_struct's values.  Each computed cell is a
    tree of depth d = tree_depth(n_win) over its values: a value passes through at most 31 additions per level (the first of a
    block is copied), so by the standard bound for recursive summation the computed cell differs from its exact sum by at most
    gamma * (the sum of its |values|), gamma = h U / (1 - h U), h = 31 d.  The four cells' |values| add up to A, exp_struct's are
    A: together 2 gamma A.  Nothing else is rounded: the sum over a is taken exactly."""
    h = 31 * tree_depth(n_win)
    gamma = Fraction(h) * Fraction(U) / (1 - Fraction(h) * Fraction(U))
    return 2 * gamma * abs_sum
