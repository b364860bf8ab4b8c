"""A numpy restatement of the posterior site map on averaged-structure profiles (include/pfmscan.h "posterior site map on
averaged-structure profiles"; rnascan_amd/csrc/pfmscan_footprint_profile.hip), COMPOSED from the rules the
family already has, nothing re-derived:

    term and has     occupancy_profile_rules.terms   (the marginal chain; joint: the letter chain first)
    occ_r            occupancy_rules.tree            (the bits of pfmscan_occupancy_profile_*)
    weight           expect_rules.weights            (the term, or t * (1.0 / occ); occ == 0.0: every weight +0.0)
    start, cover     footprint_rules.maps_of_weights (all m additions from +0.0, every one rounded)
    events           footprint_rules.events

No tolerance in any of it: the GPU tests compare bit patterns.
"""
import numpy as np

import background_rules as brules
import expect_rules as erules
import footprint_rules as frules
import occupancy_profile_rules as prules
import occupancy_rules as orules
from footprint_rules import cover_bound, events, exact_sum, total_bound  # noqa: F401  (the tests take them from here)
from occupancy_rules import same_bits  # noqa: F401

RATIO, POSTERIOR = erules.RATIO, erules.POSTERIOR
NSTRUCT = prules.NSTRUCT


def record_maps(profile, off, length, S, codes=None, R=None, mode=POSTERIOR):
    """one record under one motif -> (start [L], cover [L], occ, windows with a term); S [m][7] in the profile's STORED column
    order, R [m][8] | None (joint)"""
    m = np.asarray(S).shape[0]
    t, has = prules.terms(profile, off, length, S, codes, R)
    occ = orules.tree(t)
    w = erules.weights(t, has, occ, mode) if t.size else np.zeros(0)
    start, cover = frules.maps_of_weights(w, length, m)
    return start, cover, occ, int(has.sum())


def _stack(T):
    if T is None:
        return None
    T = np.asarray(T, dtype=np.float64)
    return T[None] if T.ndim == 2 else T


def footprint(profile, offsets, lengths, struct_tables, codes=None, seq_tables=None, mode=POSTERIOR, fill=0.0):
    """-> start, cover float64 [n_motifs][n_pos] (``fill`` where no record of the table lies), occ float64 [n_rec][n_motifs],
    windows int64 [n_rec]; struct_tables [n_motifs][m][7], seq_tables [n_motifs][m][8] | None"""
    Ss, Rs = _stack(struct_tables), _stack(seq_tables)
    n_q, n_pos = Ss.shape[0], int(np.asarray(profile).shape[0])
    start, cover = np.full((n_q, n_pos), fill, dtype=np.float64), np.full((n_q, n_pos), fill, dtype=np.float64)
    occ = np.zeros((len(offsets), n_q))
    win = np.zeros(len(offsets), dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        o, n = int(o), int(n)
        for q in range(n_q):
            start[q, o:o + n], cover[q, o:o + n], occ[r, q], win[r] = record_maps(profile, o, n, Ss[q], codes, None if Rs is None else Rs[q], mode)
    return start, cover, occ, win


class RulesEngine(object):
    """TEST-ONLY engine: ``footprint_profile``, ``footprint_profile_events`` and ``profile_colsums`` of
    rnascan_amd.scanner.HipEngine from the rules, so that the command's host logic runs without a device"""

    def __init__(self):
        self.calls = []

    def footprint_profile(self, stream, struct_tables, seq_tables, mode, want_start=True, want_cover=True):
        self.calls.append((len(stream.offsets), np.asarray(stream.profile).dtype))
        start, cover, occ, win = footprint(stream.profile, stream.offsets, stream.lengths, struct_tables, stream.codes, seq_tables, mode)
        return (start if want_start else None), (cover if want_cover else None), occ, win

    def footprint_profile_events(self, stream, struct_tables, seq_tables, mode, thr, capacity=None):
        start, cover, occ, win = self.footprint_profile(stream, struct_tables, seq_tables, mode)
        key, c, w = events(start, cover, stream.offsets, stream.lengths, thr)
        return key, c, w, occ, win

    def profile_colsums(self, stream):
        """HipEngine.profile_colsums by its rules (tests/background_rules.py): the default structure background"""
        bad = brules.first_bad(stream.profile, stream.offsets, stream.lengths)
        if bad >= 0:
            err = ValueError("bad cell")
            err.element = bad
            raise err
        return brules.colsums(stream.profile, stream.offsets, stream.lengths)

    def close(self):
        pass
