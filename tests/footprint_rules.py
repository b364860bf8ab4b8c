"""A numpy restatement of the posterior site map (include/pfmscan.h "posterior site map", DESIGN.md 5l;
rnascan_amd/csrc/pfmscan_footprint.hip), built on the rules of the family: the term of a window and the tree of the occupancy
(tests/occupancy_rules.py), the weight of a window (tests/expect_rules.py) and the joint term of two code streams
(tests/pair_rules.py) are taken from there; the two maps are stated here.  No tolerance in any of it: the GPU tests compare bit
patterns.

The two bounds at the end are derived here, not tuned.
"""
from fractions import Fraction

import numpy as np

import expect_rules as erules
import occupancy_rules as orules
import pair_rules as prules
from occupancy_rules import U, same_bits, stream, table, tree_bound  # noqa: F401  (the tests take them from here)

RATIO, POSTERIOR = erules.RATIO, erules.POSTERIOR
N_SEQ, N_STRUCT = 4, 7


# ---- the definitions -------------------------------------------------------------------------------------------------
def record_terms(codes, codes2, off, length, R, S):
    """the record's windows by the tables that are given: R alone over codes (4 letters), S alone over codes2 (7 letters),
    both the joint chain -> (t, has)"""
    if R is not None and S is not None:
        return prules.terms(codes, codes2, off, length, R, S)
    if R is not None:
        return orules.terms(codes, off, length, R, N_SEQ)
    return orules.terms(codes2, off, length, S, N_STRUCT)


def maps_of_weights(w, length, m):
    """the weights of a record's n_win windows -> (start float64 [L], cover float64 [L]).  start: the weights, then +0.0 for the
    record's last min(m - 1, L) positions.  cover: c = +0.0, then c = c + (the weight of window s, or +0.0 where there is
    none) for s = i - m + 1 .. i ascending -- m whole-array additions, each rounded"""
    L = int(length)
    w = np.asarray(w, dtype=np.float64)
    start = np.zeros(L)
    start[:w.size] = w
    cover = np.zeros(L)
    at = np.arange(L)
    with np.errstate(all="ignore"):
        for d in range(m):
            s = at - (m - 1) + d
            ok = (s >= 0) & (s < w.size)
            term = np.zeros(L)
            term[ok] = w[s[ok]]
            cover = cover + term
    return start, cover


def record_maps(codes, codes2, off, length, R, S, mode):
    """one record under one motif (or pair) -> (start [L], cover [L], occ, windows with a term)"""
    m = np.asarray(R if R is not None else S).shape[0]
    t, has = record_terms(codes, codes2, off, length, R, S)
    occ = orules.tree(t)
    w = erules.weights(t, has, occ, mode) if t.size else np.zeros(0)
    start, cover = maps_of_weights(w, length, m)
    return start, cover, occ, int(has.sum())


def _stack(T):
    if T is None:
        return None
    T = np.asarray(T, dtype=np.float64)
    return T[None] if T.ndim == 2 else T


def footprint(codes, codes2, offsets, lengths, seq_tables, struct_tables, mode, fill=0.0):
    """-> start, cover float64 [n_motifs][n_pos] (``fill`` where no record of the table lies), occ float64 [n_rec][n_motifs],
    windows int64 [n_rec]; either table stack [n_motifs][m][8] may be None"""
    Rs, Ss = _stack(seq_tables), _stack(struct_tables)
    n_q = (Rs if Rs is not None else Ss).shape[0]
    n_pos = int(np.asarray(codes if codes is not None else codes2).size)
    start, cover = np.full((n_q, n_pos), fill, dtype=np.float64), np.full((n_q, n_pos), fill, dtype=np.float64)
    occ = np.zeros((len(offsets), n_q))
    win = np.zeros(len(offsets), dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        o, n = int(o), int(n)
        for q in range(n_q):
            start[q, o:o + n], cover[q, o:o + n], occ[r, q], win[r] = record_maps(codes, codes2, o, n, None if Rs is None else Rs[q],
                                                                                  None if Ss is None else Ss[q], mode)
    return start, cover, occ, win


def events(start, cover, offsets, lengths, thr):
    """the filter of the maps: the positions inside a record with cover > thr (strict; NaN never passes) ->
    (key int64 = q * n_pos + p ascending, cover, start)"""
    n_q, n_pos = cover.shape
    inside = np.zeros(n_pos, dtype=bool)
    for o, n in zip(offsets, lengths):
        inside[int(o):int(o) + int(n)] = True
    with np.errstate(invalid="ignore"):
        q, p = np.nonzero((cover > thr) & inside[None, :])
    return q.astype(np.int64) * n_pos + p, cover[q, p], start[q, p]


def by_letter(start_row, codes_row, has, m, n_letters):
    """the rows the expected counts sum, from a record's start map: X[k * n_letters + c][s] = start[s] where window s has a term
    and the letter under its column k is c -> float64 [m * n_letters][n_win]"""
    n_win = int(has.size)
    c = np.asarray(codes_row) & 7
    X = np.zeros((m * n_letters, n_win))
    for k in range(m):
        ck = c[k:k + n_win]
        for l in range(n_letters):
            X[k * n_letters + l] = np.where(has & (ck == l), start_row[:n_win], 0.0)
    return X


class RulesEngine(object):
    """TEST-ONLY engine: ``footprint`` and ``footprint_events`` of rnascan_amd.scanner.HipEngine from the rules above, so that
    the command's host logic runs without a device"""

    @staticmethod
    def _streams(stream, seq_tables, struct_tables):
        codes2 = stream.codes2 if getattr(stream, "codes2", None) is not None else (stream.codes if seq_tables is None else None)
        return stream.codes, codes2

    def footprint(self, stream, seq_tables, struct_tables, mode, want_start=True, want_cover=True):
        codes, codes2 = self._streams(stream, seq_tables, struct_tables)
        start, cover, occ, win = footprint(codes, codes2, stream.offsets, stream.lengths, seq_tables, struct_tables, mode)
        return (start if want_start else None), (cover if want_cover else None), occ, win

    def footprint_events(self, stream, seq_tables, struct_tables, mode, thr, capacity=None):
        start, cover, occ, win = self.footprint(stream, seq_tables, struct_tables, mode)
        key, c, w = events(start, cover, stream.offsets, stream.lengths, thr)
        return key, c, w, occ, win

    def close(self):
        pass


# ---- bounds ----------------------------------------------------------------------------------------------------------
def gamma(k):
    """k rounded operations on non-negative values: relative error at most k U / (1 - k U)"""
    return k * U / (1.0 - k * U)


def cover_bound(n_win, m):
    """POSTERIOR mode, occ finite and > 0: cover <= cover_bound(n_win, m) at every position.

    occ = T (1 + a), |a| <= tree_bound(n_win), T the exact sum of the record's terms; v = (1 / occ)(1 + b), |b| <= U (one rounded
    division); w_s = t_s v (1 + d_s), |d_s| <= U (one rounded product).  So the EXACT sum of all weights is at most
    (T / occ)(1 + U)(1 + U) = 1 + tree_bound + 2 U to first order.  A cover is a sub-sum of the weights (they are >= 0) made
    with m - 1 rounded additions (the first adds to +0.0, which is exact): at most (1 + (m - 1) U) times its exact value.
    Together 1 + tree_bound + (m + 1) U."""
    return 1.0 + tree_bound(n_win) + (m + 1) * U


def total_bound(m):
    """any mode, finite weights: |sum_i cover_i - m sum_s w_s| <= total_bound(m) * m sum_s w_s, both sums exact.

    Window s lies over the m positions s .. s + m - 1, all inside the record, so the exact covers add up to m times the exact
    sum of the weights.  A computed cover is m - 1 rounded additions of non-negative values: within gamma(m - 1) relative of
    its exact value, and so is their sum."""
    return gamma(m - 1)


def exact_sum(x):
    return sum((Fraction(float(v)) for v in np.asarray(x, dtype=np.float64).ravel()), Fraction(0))
