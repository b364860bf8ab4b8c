"""A numpy restatement of the threshold-free mutagenesis (include/pfmscan.h "threshold-free mutagenesis", DESIGN.md 5m;
rnascan_amd/csrc/pfmscan_mutocc.hip), built on the rules of the family: the term of a window and the tree of the occupancy
(tests/occupancy_rules.py), the ratio weight of a window (tests/expect_rules.py) and the cover of a position
(tests/footprint_rules.py) are taken from there; the map of the four letters and its events are stated here.  No tolerance in
any of it: the GPU tests compare bit patterns.

Two identities tie the map to what is already pinned, and tests/test_mutocc_cpu.py checks both by really mutating the stream:
  * the column of the letter the record holds, local[i][c_i], is bit for bit the ``cover`` of ``footprint_rules`` in RATIO mode
    on the same stream and table: the same terms, added in the same order from +0.0;
  * for every letter a, local[i][a] is bit for bit that cover at i of the stream with a written at i: the windows over i of the
    mutated stream are the u(s) below, and the cover adds them in ascending s.

The bound at the end is derived here, not tuned.
"""
import math
from fractions import Fraction

import numpy as np

import expect_rules as erules
import footprint_rules as frules
import occupancy_rules as orules
from footprint_rules import exact_sum, gamma  # noqa: F401  (the tests take them from here)
from occupancy_rules import U, same_bits, stream, table, tree_bound  # noqa: F401

RATIO = erules.RATIO
N_SEQ = 4


# ---- the definitions -------------------------------------------------------------------------------------------------
def record_local(codes, off, length, R):
    """one record under one motif -> local float64 [L][4].  For a position i that holds a letter and a letter a: x = +0.0, then
    x = x + u(s) for s = i - m + 1 .. i ascending, every addition rounded; u(s) = +0.0 when the window leaves the record or
    holds a code >= 4 at a position other than i, else R[0][.] * R[1][.] * ... left to right with a at i, every product rounded.
    A position that holds no letter has four NaN."""
    return records_local(codes, [off], [length], R)[int(off):int(off) + int(length)]


def records_local(codes, offsets, lengths, R, fill=np.nan):
    """the records of a stream under one motif, all at once -> local float64 [n_pos][4], ``fill`` where no record lies.  The
    factors before position i do not depend on the letter: they are multiplied once and the four letters go on from there,
    which is the same products in the same order."""
    R = np.asarray(R, dtype=np.float64)
    m = R.shape[0]
    c = (np.asarray(codes) & 7).astype(np.int64)
    p = np.concatenate([np.arange(int(o), int(o) + int(n)) for o, n in zip(offsets, lengths)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    i = np.concatenate([np.arange(int(n)) for n in lengths] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    L = np.concatenate([np.full(int(n), int(n)) for n in lengths] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    rows = np.zeros((p.size, 4))
    with np.errstate(all="ignore"):
        for j in range(m - 1, -1, -1):                             # s = i - j ascending
            s = i - j
            at = np.flatnonzero((s >= 0) & (s <= L - m))           # the window lies inside the record: inside the stream
            W = c[(p[at] - j)[:, None] + np.arange(m)[None, :]]    # its codes
            others = np.ones(at.size, dtype=bool)
            for k in range(m):
                if k != j:
                    others &= W[:, k] < N_SEQ
            pre = None
            for k in range(j):                                     # whole arrays: one rounded product per window and k
                pre = R[0][W[:, 0]] if k == 0 else pre * R[k][W[:, k]]
            for a in range(4):
                x = np.full(at.size, R[0][a]) if j == 0 else pre * R[j][a]
                for k in range(j + 1, m):
                    x = x * R[k][W[:, k]]
                u = np.zeros(p.size)
                u[at] = np.where(others, x, 0.0)
                rows[:, a] = rows[:, a] + u
    rows[c[p] >= N_SEQ] = np.nan
    local = np.full((c.size, 4), fill, dtype=np.float64)
    local[p] = rows
    return local


def mutocc(codes, offsets, lengths, tables, fill=np.nan):
    """-> local float64 [n_motifs][n_pos][4] (``fill`` where no record of the table lies), occ float64 [n_rec][n_motifs],
    windows int64 [n_rec]; tables [n_motifs][m][8] of one width (or one [m][8])"""
    tables = np.asarray(tables, dtype=np.float64)
    if tables.ndim == 2:
        tables = tables[None]
    local = np.stack([records_local(codes, offsets, lengths, tables[q], fill) for q in range(tables.shape[0])])
    occ, win = orules.occupancy(codes, offsets, lengths, tables, N_SEQ)
    return local, occ, win


def classify(ref, alt, occ, frac):
    """-> (delta = alt - ref one rounded subtraction, gain = delta > lim, loss = delta < -lim with lim = frac * occ one rounded
    product; both compares strict, NaN never passes)"""
    with np.errstate(all="ignore"):
        delta = np.asarray(alt, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
        lim = np.float64(frac) * np.asarray(occ, dtype=np.float64)
        return delta, delta > lim, delta < -lim


def events(local, codes, offsets, lengths, occ, frac):
    """the filter of the map: (q, p, a != c_p) inside a record with a gain or a loss -> (key int64 = (q * n_pos + p) * 4 + a
    ascending, alt = local[q][p][a], ref = local[q][p][c_p])"""
    if not frac >= 0:
        raise ValueError("frac is negative or not a number")
    n_q, n_pos, _ = local.shape
    c = np.asarray(codes) & 7
    keys, alts, refs = [], [], []
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        o, n = int(o), int(n)
        p = o + np.flatnonzero(c[o:o + n] < N_SEQ)
        for q in range(n_q):
            ref = local[q, p, c[p]]
            for a in range(4):
                _, gain, loss = classify(ref, local[q, p, a], occ[r, q], frac)
                hit = (gain | loss) & (c[p] != a)
                keys.append((q * n_pos + p[hit]) * 4 + a)
                alts.append(local[q, p[hit], a])
                refs.append(ref[hit])
    key = np.concatenate(keys).astype(np.int64) if keys else np.zeros(0, dtype=np.int64)
    alt = np.concatenate(alts) if alts else np.zeros(0)
    ref = np.concatenate(refs) if refs else np.zeros(0)
    order = np.argsort(key, kind="stable")
    return key[order], alt[order], ref[order]


def cover_with(codes, off, length, R, i, a):
    """brute force: write a at position i of the record and take ``footprint_rules``'s RATIO cover there"""
    mutated = np.array(codes, copy=True)
    mutated[int(off) + i] = a
    _, cover, _, _ = frules.record_maps(mutated, None, off, length, R, None, RATIO)
    return cover[i]


class RulesEngine(object):
    """TEST-ONLY engine: ``mutocc`` and ``mutocc_events`` of rnascan_amd.scanner.HipEngine from the rules above, so that the
    command's host logic runs without a device"""

    def mutocc(self, stream, ratio_tables):
        return mutocc(stream.codes, stream.offsets, stream.lengths, ratio_tables)

    def mutocc_events(self, stream, ratio_tables, frac, capacity=None):
        local, occ, win = self.mutocc(stream, ratio_tables)
        key, alt, ref = events(local, stream.codes, stream.offsets, stream.lengths, occ, frac)
        return key, alt, ref, occ, win

    def close(self):
        pass


# ---- the bound -------------------------------------------------------------------------------------------------------
def occupancy_alt(occ, local_alt, local_ref):
    """the command's Occupancy.Alt: the exact value of occ + local_alt - local_ref rounded once, not below 0"""
    return max(math.fsum([float(occ), float(local_alt), -float(local_ref)]), 0.0)


def occupancy_alt_bound(n_win, m, T, Lref, Lalt, occ_alt):
    """finite non-negative tables: |Occupancy.Alt - T'| <= this, T' the exact sum of the terms of the MUTATED record.

    The terms are doubles; T is the exact sum of the record's, Lref the exact sum of those of the windows over the position,
    Lalt the same after the change.  The windows that do not lie over the position are untouched, so T' = T - Lref + Lalt
    exactly.  occ = T (1 + a), |a| <= tree_bound(n_win) (the tree).  local_ref and local_alt are at most m non-negative terms
    added from +0.0 with m - 1 roundings that count (the first addition is exact): each within gamma(m - 1) relative of Lref and
    Lalt.  ``math.fsum`` adds the three doubles exactly and rounds once: U |Occupancy.Alt|; the clamp at 0 only moves the value
    towards T' >= 0.  Together: tree_bound(n_win) T + gamma(m - 1) (Lref + Lalt) + U |Occupancy.Alt|."""
    return float(tree_bound(n_win) * Fraction(T) + Fraction(gamma(m - 1)) * (Fraction(Lref) + Fraction(Lalt))) + U * abs(float(occ_alt))
