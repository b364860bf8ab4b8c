"""A numpy restatement of the occupancy (include/pfmscan.h "occupancy"; rnascan_amd/csrc/pfmscan_occupancy.hip):
the ratio table of a PFM, the term of a window as a sequential fp64 product, the left-aligned summation tree of fan-in 32
anchored at the record's first window, and Windows.  No tolerance in any of it: the GPU tests compare bit patterns.

The two bounds at the end tie the new quantity to arithmetic the project already pins; they are derived here, not tuned.
"""
import math

import numpy as np

FANIN = 32
SEP = 7
U = 2.0 ** -53                       # unit roundoff of binary64


# ---- the definitions -------------------------------------------------------------------------------------------------
def ratio_table(counts, background=None, pseudocount=0.0):
    """counts [m][n_letters] (column c = code c) -> R float64 [m][8]: p / b where that is > 0, else +0.0; b == 0: +inf if
    p > 0 else NaN; columns >= n_letters NaN.  p and b are normalised as pssm.normalize / pssm.log_odds normalise them (sums
    taken left to right)."""
    M = np.asarray(counts, dtype=np.float64) + float(pseudocount)
    m, n = M.shape
    total = np.zeros(m)
    for k in range(n):
        total = total + M[:, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        P = M / total[:, None]
    if background is None:
        b = [1.0 / n] * n
    else:
        s = 0.0
        for k in range(n):
            s += float(background[k])
        b = [float(background[k]) / s for k in range(n)]
    R = np.full((m, 8), np.nan)
    for c in range(n):
        for j in range(m):
            p = float(P[j, c])
            if b[c] > 0:
                q = p / b[c]
                R[j, c] = q if q > 0 else 0.0
            else:
                R[j, c] = math.inf if p > 0 else math.nan
    return R


def terms(codes, off, length, R, n_letters):
    """the record's windows in order -> (t float64 [n_win] with +0.0 where the window has no term, has bool [n_win])"""
    R = np.asarray(R, dtype=np.float64)
    m = R.shape[0]
    n_win = max(int(length) - m + 1, 0)
    if n_win == 0:
        return np.zeros(0), np.zeros(0, dtype=bool)
    c = np.asarray(codes[int(off):int(off) + int(length)]) & 7
    with np.errstate(all="ignore"):
        t = R[0][c[0:n_win]]
        for k in range(1, m):
            t = t * R[k][c[k:k + n_win]]                  # whole arrays: one rounded product per window and k
    has = np.ones(n_win, dtype=bool)
    for k in range(m):
        has &= c[k:k + n_win] < n_letters
    return np.where(has, t, 0.0), has


def tree(t):
    """left-aligned tree of fan-in 32: zero-pad to a multiple of 32 (x + 0.0 is exact for +0.0, positive, +inf and NaN),
    31 array additions per level, until one value is left"""
    a = np.asarray(t, dtype=np.float64)
    if a.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        while a.size > 1:
            pad = (-a.size) % FANIN
            if pad:
                a = np.concatenate([a, np.zeros(pad)])
            a = a.reshape(-1, FANIN)
            s = a[:, 0]
            for i in range(1, FANIN):
                s = s + a[:, i]
            a = s
    return float(a[0])


def depth(n_win):
    d = 0
    while n_win > 1:
        n_win = -(-n_win // FANIN)
        d += 1
    return d


def occupancy(codes, offsets, lengths, tables, n_letters):
    """-> occ float64 [n_rec][n_motifs], windows int64 [n_rec]; tables [n_motifs][m][8] of one width"""
    tables = np.asarray(tables, dtype=np.float64)
    if tables.ndim == 2:
        tables = tables[None]
    occ = np.zeros((len(offsets), tables.shape[0]))
    win = np.zeros(len(offsets), dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(tables.shape[0]):
            t, has = terms(codes, o, n, tables[q], n_letters)
            occ[r, q] = tree(t)
            win[r] = int(has.sum())
    return occ, win


def same_bits(a, b):
    """float64 bit patterns equal, NaN == NaN whatever its payload"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


# ---- streams and tables for the tests --------------------------------------------------------------------------------
def stream(rng, lengths, n_letters=4, foreign=0.0, case=False):
    """records of the given lengths, one separator after each -> (codes uint8, offsets int64, lengths int64).  ``foreign``:
    share of positions that hold a code >= n_letters; ``case``: bit 3 set on a third of the letters (lower-case structure letters)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.size, dtype=np.int64)
    if lengths.size > 1:
        offsets[1:] = np.cumsum(lengths[:-1] + 1)
    codes = np.full(int((lengths + 1).sum()), SEP, dtype=np.uint8)
    for o, n in zip(offsets, lengths):
        c = rng.integers(0, n_letters, size=int(n)).astype(np.uint8)
        if foreign > 0:
            bad = rng.random(int(n)) < foreign
            c[bad] = rng.integers(n_letters, 8, size=int(bad.sum())).astype(np.uint8)
        if case:
            low = (rng.random(int(n)) < 1.0 / 3) & (c < n_letters)
            c[low] |= 8
        codes[o:o + n] = c
    return codes, offsets, lengths


def table(rng, m, n_letters=4, lo=0.2, hi=3.0):
    """a ratio table with ratios drawn log-uniformly from [lo, hi]"""
    R = np.full((m, 8), np.nan)
    R[:, :n_letters] = np.exp(rng.uniform(math.log(lo), math.log(hi), size=(m, n_letters)))
    return R


# ---- bounds ----------------------------------------------------------------------------------------------------------
def term_log2_bound(m, cells):
    """|log2(term) - fsum(cells)| for a finite positive table whose products stay normal, cells = the window's m PSSM cells.

    The term is m - 1 rounded products of the exact ratios: term = prod(R_k) * prod(1 + d_i), |d_i| <= U, so
    log2(term) is off by at most (m - 1) * U / ln 2 * (1 + U).  A PSSM cell is log(q) / log(2) in doubles: a rounded log
    (libm: within 1 ulp = 2 U relative), the rounded constant log(2) (U) and a rounded quotient (U) -- at most 4 U |cell|
    each, m of them.  fsum adds them exactly and rounds once (U |sum|), and log2 of the term is one more rounded log
    (2 U |log2 term|, and |log2 term| <= sum |cell| + the first error).  Together:"""
    s = float(np.sum(np.abs(cells)))
    return U * ((m - 1) / math.log(2.0) * (1 + U) + 4 * s + s + 2 * (s + 1))


def tree_bound(n_win):
    """relative error of the tree against the exact sum of non-negative terms: every term passes through at most 31
    rounded additions per level"""
    return depth(n_win) * (FANIN - 1) * U
