"""TEST-ONLY helpers of the site-profile tests (CPU and GPU): the oracle-backed engine whose ``site_sums`` is the numpy
restatement (tests/sites_rules.py), beside the restated ``profile_colsums`` of tests/background_helpers.py."""
import numpy as np

import background_helpers
from background_helpers import COLUMNS, random_rows, write_fasta, write_profile
import sites_rules as rules
from engines import OracleEngine


class RulesEngine(background_helpers.RulesEngine):
    """the oracle-backed engine + site_sums from the restated rules (same contract as HipEngine.site_sums)"""

    def site_sums(self, stream, pos, m, flank=0, letters=True, profile=True):
        letters = bool(letters) and stream.codes is not None
        profile = bool(profile) and stream.profile is not None
        if not letters and not profile:
            raise ValueError("the stream has neither the codes nor the profile asked for")
        if m + 2 * flank > 4096:
            raise ValueError("width + 2 x flank exceeds PFMSCAN_MAX_WIDTH")
        if profile:
            bad = rules.first_bad(stream.profile, pos, stream.offsets, stream.lengths, m, flank)
            if bad >= 0:
                err = ValueError("bad cell")
                err.element = bad
                raise err
        return rules.site_sums(stream.profile if profile else None, stream.codes if letters else None, pos, stream.offsets,
                               stream.lengths, m, flank)


assert issubclass(RulesEngine, OracleEngine)


def site_windows(stream, pos, m, flank=0):
    """per hit the rows [W] of its columns and whether they count (a plain loop: the checker of the checker)"""
    W = m + 2 * flank
    rec, _ = stream.locate(np.asarray(pos, dtype=np.int64))
    x = np.asarray(pos, dtype=np.int64)[:, None] - flank + np.arange(W)
    lo = stream.offsets[rec][:, None]
    return x, (x >= lo) & (x < lo + stream.lengths[rec][:, None])


SITE = "AAAGGCTCTTTTCAGAGC"                  # the SLBP site: the shipped sequence PFM scores it above the default -m


def write_inputs(tmp_path, n=31, seed=5, orders=None):
    """a FASTA whose records hold the SLBP site here and there, a profile directory and a packed store of the same records"""
    rng = np.random.default_rng(seed)
    d = tmp_path / "avg"
    d.mkdir(parents=True)
    recs = []
    for i in range(n):
        body = "".join(rng.choice(list("ACGU"), size=int(rng.integers(20, 260))))
        if i % 3 != 1:
            at = int(rng.integers(0, len(body)))
            body = body[:at] + SITE + body[at:]
        if i % 4 == 0:
            body = SITE[3:] + body + SITE[:-2] + ("N" if i % 8 == 0 else "")      # sites at the very ends: flanks hang over
        recs.append(("k%02d" % i, body))
        order = orders[i % len(orders)] if orders else COLUMNS
        p = random_rows(rng, len(body))
        write_profile(str(d / ("structure.k%02d.txt" % i)), p[:, [COLUMNS.index(c) for c in order]], order)
    fa = str(tmp_path / "seqs.fa")
    write_fasta(fa, recs)
    sdir = str(tmp_path / "store")
    if not orders:
        from rnascan_amd import store
        store.build_store(str(d), sdir)
    return fa, str(d), sdir
