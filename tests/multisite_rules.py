"""A numpy restatement of the multi-site model (include/pfmscan.h "multi-site model", DESIGN.md 5n;
rnascan_amd/csrc/pfmscan_multisite.hip).  The term of a window -- a sequence table alone, a structure table alone, or the pair
chain of two code streams -- is ``footprint_rules.record_terms``, the cover of a position ``footprint_rules.maps_of_weights``;
the recurrences over a record are stated here.  Every product and addition is one rounded fp64 operation in a fixed order (the
loops below run on Python floats: IEEE binary64, one rounding each, no exception on overflow).  No tolerance in any of it: the
GPU tests compare bit patterns.

The bounds at the end are derived here, not tuned.
"""
import numpy as np

import footprint_rules as frules
from footprint_rules import U, events, exact_sum, gamma, same_bits, stream, table  # noqa: F401  (the tests take them from here)

N_SEQ, N_STRUCT = frules.N_SEQ, frules.N_STRUCT


# ---- the definitions -------------------------------------------------------------------------------------------------
def activities(t, lam):
    """a_s = t_s * lam, one rounded product per window (a window without a term has t_s = +0.0)"""
    lam = float(lam)
    return [float(x) * lam for x in np.asarray(t, dtype=np.float64)]


def forward(a, L, m):
    """F[0] = 1.0; F[i] = F[i-1] + (a[i-m] * F[i-m] if i >= m else +0.0) -> F as a list of L + 1 floats"""
    F = [1.0] * (L + 1)
    for i in range(1, L + 1):
        g = a[i - m] * F[i - m] if i >= m else 0.0
        F[i] = F[i - 1] + g
    return F


def backward(a, L, m):
    """B[L] = 1.0; B[i] = B[i+1] + (a[i] * B[i+m] if i <= L - m else +0.0) -> B as a list of L + 1 floats"""
    B = [1.0] * (L + 1)
    for i in range(L - 1, -1, -1):
        h = a[i] * B[i + m] if i <= L - m else 0.0
        B[i] = B[i + 1] + h
    return B


def posteriors(a, F, B, L, m):
    """v = 1.0 / Z one rounded division; start[s] = ((F[s] * a[s]) * B[s+m]) * v for the record's windows; nsites = +0.0, then
    nsites + start[s] for s = n_win - 1 down to 0 -> (start float64 [n_win], Z, nsites)"""
    n_win = max(L - m + 1, 0)
    Z = F[L]
    with np.errstate(all="ignore"):
        v = float(np.float64(1.0) / np.float64(Z))
    start = [((F[s] * a[s]) * B[s + m]) * v for s in range(n_win)]
    n = 0.0
    for s in range(n_win - 1, -1, -1):
        n = n + start[s]
    return np.array(start, dtype=np.float64), Z, n


def model_of_terms(t, lam, L, m):
    """a record's terms -> (start [L], cover [L], Z, nsites)"""
    a = activities(t, lam)
    F, B = forward(a, L, m), backward(a, L, m)
    w, Z, n = posteriors(a, F, B, L, m)
    start, cover = frules.maps_of_weights(w, L, m)
    return start, cover, Z, n


def record_model(codes, codes2, off, length, R, S, lam):
    """one record under one motif (or pair) -> (start [L], cover [L], Z, nsites, windows with a term)"""
    m = np.asarray(R if R is not None else S).shape[0]
    t, has = frules.record_terms(codes, codes2, off, length, R, S)
    start, cover, Z, n = model_of_terms(t, lam, int(length), m)
    return start, cover, Z, n, int(has.sum())


def multisite(codes, codes2, offsets, lengths, seq_tables, struct_tables, lam, fill=0.0):
    """-> start, cover float64 [n_motifs][n_pos] (``fill`` where no record of the table lies), z, nsites float64
    [n_rec][n_motifs], windows int64 [n_rec]; either table stack [n_motifs][m][8] may be None; lam float64 [n_rec]"""
    Rs, Ss = frules._stack(seq_tables), frules._stack(struct_tables)
    n_q = (Rs if Rs is not None else Ss).shape[0]
    n_pos = int(np.asarray(codes if codes is not None else codes2).size)
    start, cover = np.full((n_q, n_pos), fill, dtype=np.float64), np.full((n_q, n_pos), fill, dtype=np.float64)
    z, ns = np.zeros((len(offsets), n_q)), np.zeros((len(offsets), n_q))
    win = np.zeros(len(offsets), dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        o, n = int(o), int(n)
        for q in range(n_q):
            start[q, o:o + n], cover[q, o:o + n], z[r, q], ns[r, q], win[r] = record_model(
                codes, codes2, o, n, None if Rs is None else Rs[q], None if Ss is None else Ss[q], lam[r])
    return start, cover, z, ns, win


class RulesEngine(object):
    """TEST-ONLY engine: ``multisite`` and ``multisite_events`` of rnascan_amd.scanner.HipEngine from the rules above, so that
    the command's host logic runs without a device"""

    def multisite(self, stream, seq_tables, struct_tables, lam, want_start=True, want_cover=True):
        codes, codes2 = frules.RulesEngine._streams(stream, seq_tables, struct_tables)
        start, cover, z, ns, win = multisite(codes, codes2, stream.offsets, stream.lengths, seq_tables, struct_tables, np.asarray(lam, dtype=np.float64))
        return (start if want_start else None), (cover if want_cover else None), z, ns, win

    def multisite_events(self, stream, seq_tables, struct_tables, lam, thr, capacity=None):
        start, cover, z, ns, win = self.multisite(stream, seq_tables, struct_tables, lam)
        key, c, w = events(start, cover, stream.offsets, stream.lengths, thr)
        return key, c, w, z, ns, win

    def close(self):
        pass


# ---- bounds ----------------------------------------------------------------------------------------------------------
# All of them for finite, non-negative activities and a Z that stays finite: every operand is then non-negative, a rounded
# operation multiplies its exact result by (1 + d), |d| <= U, and k of them in a chain stay within gamma(k) of the exact value.
def z_bound(L):
    """relative error of F[i] (i <= L), of Z = F[L] and of B[i] against the exact sum over configurations.

    By induction F[i] carries at most 2 i rounded operations: F[i-1] (2 (i - 1)) plus this step's product and addition, and
    the product's operand F[i-m] carries fewer than F[i-1] does.  The same walk mirrored gives B."""
    return gamma(2 * L)


def start_bound(L):
    """relative error of start[s] against the exact posterior: F[s] (2 s operations), B[s+m] (2 (L - s - m)), Z (2 L), the
    division and the three products: at most 4 L + 4 - 2 m <= 4 L + 4 operations"""
    return gamma(4 * L + 4)


def cover_bound(L, m):
    """cover <= cover_bound at every position: the exact posteriors of the windows over one position belong to disjoint events
    and add up to at most 1; each computed start is within start_bound of its own, and the m - 1 rounded additions (the first
    adds to +0.0, exact) add gamma(m - 1)"""
    return 1.0 + gamma(4 * L + 4 + m)


def nsites_bound(n_win):
    """relative error of nsites against the exact sum of the COMPUTED start weights: n_win - 1 rounded additions of
    non-negative values (the first adds to +0.0)"""
    return gamma(max(n_win - 1, 0))
