"""A numpy restatement of the multi-site model on averaged-structure profiles (include/pfmscan.h "multi-site model on
averaged-structure profiles"; k_ms_profile_terms in rnascan_amd/csrc/pfmscan_multisite.hip), COMPOSED from the rules
the family already has, nothing re-derived:

    term and has           occupancy_profile_rules.terms   (the marginal chain; joint: the letter chain first)
    a, F, B, Z, start,     multisite_rules.model_of_terms  (a_s = t_s * lam, both recurrences, the posteriors, the cover)
    cover, nsites
    events                 footprint_rules.events

No tolerance in any of it: the GPU tests compare bit patterns.  Profile cells may be negative or not finite (-u / -B): nothing
here treats them specially, every operation is a rounded fp64 operation in the stated order and Z, start and cover are what IEEE
makes of them; what to do with a Z that is not positive and finite is the command's decision.
"""
import numpy as np

import background_rules as brules
import multisite_rules as mrules
import occupancy_profile_rules as prules
from multisite_rules import events, exact_sum, gamma, nsites_bound, same_bits  # noqa: F401  (the tests take them from here)
# The three bounds below hold for FINITE, NON-NEGATIVE activities and a Z that stays finite only (multisite_rules.py derives
# them from operands of one sign): on profiles that is non-negative finite rows, tables and lam.  With a negative cell they say
# nothing.  They bound the model against its exact value OVER THE COMPUTED TERMS; a term's own rounding is
# occupancy_profile_rules.term_bound.
from multisite_rules import cover_bound, start_bound, z_bound  # noqa: F401
from occupancy_profile_rules import term_bound  # noqa: F401

NSTRUCT = prules.NSTRUCT


def record_model(profile, off, length, S, lam, codes=None, R=None):
    """one record under one motif -> (start [L], cover [L], Z, nsites, windows with a term); S [m][7] in the profile's STORED
    column order, R [m][8] | None (joint)"""
    m = np.asarray(S).shape[0]
    t, has = prules.terms(profile, off, length, S, codes, R)
    start, cover, Z, n = mrules.model_of_terms(t, lam, int(length), m)
    return start, cover, Z, n, int(has.sum())


def _stack(T):
    if T is None:
        return None
    T = np.asarray(T, dtype=np.float64)
    return T[None] if T.ndim == 2 else T


def multisite(profile, offsets, lengths, struct_tables, codes=None, seq_tables=None, lam=None, fill=0.0):
    """-> start, cover float64 [n_motifs][n_pos] (``fill`` where no record of the table lies), z, nsites float64
    [n_rec][n_motifs], windows int64 [n_rec]; struct_tables [n_motifs][m][7], seq_tables [n_motifs][m][8] | None, lam float64
    [n_rec]"""
    Ss, Rs = _stack(struct_tables), _stack(seq_tables)
    n_q, n_pos = Ss.shape[0], int(np.asarray(profile).shape[0])
    start, cover = np.full((n_q, n_pos), fill, dtype=np.float64), np.full((n_q, n_pos), fill, dtype=np.float64)
    z, ns = np.zeros((len(offsets), n_q)), np.zeros((len(offsets), n_q))
    win = np.zeros(len(offsets), dtype=np.int64)
    with np.errstate(all="ignore"):
        for r, (o, n) in enumerate(zip(offsets, lengths)):
            o, n = int(o), int(n)
            for q in range(n_q):
                start[q, o:o + n], cover[q, o:o + n], z[r, q], ns[r, q], win[r] = record_model(
                    profile, o, n, Ss[q], lam[r], codes, None if Rs is None else Rs[q])
    return start, cover, z, ns, win


class RulesEngine(object):
    """TEST-ONLY engine: ``multisite_profile``, ``multisite_profile_events`` and ``profile_colsums`` of
    rnascan_amd.scanner.HipEngine from the rules, so that the command's host logic runs without a device"""

    def __init__(self):
        self.calls = []

    def multisite_profile(self, stream, struct_tables, seq_tables, lam, want_start=True, want_cover=True):
        self.calls.append((len(stream.offsets), np.asarray(stream.profile).dtype))
        start, cover, z, ns, win = multisite(stream.profile, stream.offsets, stream.lengths, struct_tables, stream.codes, seq_tables,
                                             np.asarray(lam, dtype=np.float64))
        return (start if want_start else None), (cover if want_cover else None), z, ns, win

    def multisite_profile_events(self, stream, struct_tables, seq_tables, lam, thr, capacity=None):
        start, cover, z, ns, win = self.multisite_profile(stream, struct_tables, seq_tables, lam)
        key, c, w = events(start, cover, stream.offsets, stream.lengths, thr)
        return key, c, w, z, ns, win

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
