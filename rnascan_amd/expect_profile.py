"""Expected counts on averaged-structure profiles: the structural context of a motif's sites, without a threshold.

    python -m rnascan_amd.expect_profile -q struct.pfm [...] avgdir_or_store/ -o PREFIX
    python -m rnascan_amd.expect_profile -p seq.pfm -q struct.pfm [...] seqs.fa avgdir_or_store/ -o PREFIX
    python -m rnascan_amd.expect_profile -p seq.pfm [...] seqs.fa avgdir_or_store/ -o PREFIX
        [-C c] [-u | -b bg | -B bg] [--weight posterior|ratio] [--iterations N] [--all-motifs]
        [--pairing aligned|positional] [--profile-dtype float32|float64] [--batch-records n]
        [--merge auto|device|host] [--device d]

Every window of every record is weighted as ``expect`` weights it (``--weight``), by the structure motif's marginal ratios
over the averaged-structure profile (``-q`` alone), by the sequence motif's ratios over the FASTA's letters (``-p`` alone), or
by their product, the ratio behind ``LogOdds.SeqStruct`` (``-p`` with ``-q``) -- the three weights of ``occupancy``.  Under
these weights the profile's ROWS are added up: ``E[k][c]`` is the sum over the windows of ``w * r[s + k][c]``, the expected
amount of structural context ``c`` under motif column ``k``.  It is the threshold-free form of what ``sites``
sums under hits; on profiles with a single 1 per row it is ``expect``'s count of structure letters.  It is NOT the posterior
of the letter given the motif (``r * S / d``), which this does not compute.  With ``-p`` the letters are counted too, as
``expect`` counts them, under the same weights.  The weights and per-record sums are made on the GPU, bit for bit by the
rules of DESIGN.md 5g / 5h / 5i; the records are added up exactly, on the device or with ``math.fsum`` on the host
(``--merge``, DESIGN.md 5k: the same bytes; a negative profile cell, which the device's accumulators cannot hold, sends
``auto`` to the host and ends ``device`` with exit 1), so the bytes written do not depend on ``--batch-records`` or on the
order of the records.

``PREFIX.expected.struct.txt``: the structure matrix as a raw-sum PFM that ``-q`` reads; ``PREFIX.expected.seq.txt`` (with
``-p``): the sequence matrix as a raw-sum PFM that ``-p`` reads.  Both are multi-PFM libraries in pair order with
``--all-motifs`` (pairs named as the site profiles name them), the first motif (pair) otherwise.  ``PREFIX.summary.txt``
has ``expect``'s columns.

Records and profiles are matched by id, two libraries are paired, widths are checked, the structure background defaults to
the profiles' own and the rows' storage is chosen exactly as ``occupancy`` does it (the same code).  A directory whose
files store their columns in different orders is summed per run of equal order, each mapped to the profile's letters before
the records are added.

``--iterations N``: every given PFM is replaced by its own expected matrix, normalised with the same pseudocount against the
same background, and the pass is run again; with ``-p`` alone the sequence matrix is fed back and the structure matrix is
the last pass's.  ``--iterations 2`` writes the bytes of a run on the outputs of a run.  Refused with ``--pairing
positional``, under which the written columns are not the ones the PFM's letters were paired with.

Not supported: ``--flank``, two-FASTA pairs, ``--gpus``, other priors.
"""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np

from . import expect, fasta, pack

BATCH_RECORDS = expect.BATCH_RECORDS


NOT_FINITE = ("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
              "(a ratio of the motif or a cell of the profile is; check the background and the pseudocount)")


def run(engine, recs, profiles, seq_odds, struct_odds, pairs, mode, pairing="aligned", batch_records=BATCH_RECORDS, merge="host"):
    """one pass -> {pair id: (E_struct float64 [m][7] in sites.STRUCT_ORDER, E_seq float64 [m][4] in code order | None,
    records, skipped, windows, log2 likelihood)}.  ``pairs``: [(sequence id | None, structure id | None)]; ``recs``: the
    FASTA's records in the profiles' order, or None (structure only).  ``merge``: where the records are added up
    (expect.MERGES); the result does not depend on it."""
    args = (engine, recs, profiles, seq_odds, struct_odds, pairs, mode, pairing, batch_records)
    return expect.with_merge(merge, expect.merge_route(engine, merge, "expect_profile_merged"), lambda: run_merged(*args), lambda: run_host(*args))


class _Folded(object):
    """the structure accumulators of one width, cell axis in the WRITTEN letters' order (sites.STRUCT_ORDER).  The device adds
    in the run's stored column order: the runs of one order share an accumulator, which is folded in -- its columns mapped to
    the letters -- when the order changes and at the end"""

    def __init__(self, n_motifs, m):
        self.total = expect.new_acc(n_motifs, m)
        self.n_motifs, self.m = n_motifs, m
        self.order, self.acc = None, None

    def current(self, to_letters):
        if self.order != to_letters:
            self.fold()
            self.order, self.acc = list(to_letters), expect.new_acc(self.n_motifs, self.m)
        return self.acc

    def fold(self):
        from . import _lib
        if self.acc is not None:
            cells = self.acc.reshape(self.n_motifs, _lib.SITE_LIMBS, self.m, _lib.NCODE)
            _lib.site_acc_add(self.total, np.ascontiguousarray(cells[:, :, :, self.order + [7]]).reshape(self.total.shape))
        self.order, self.acc = None, None
        return self.total


def run_merged(engine, recs, profiles, seq_odds, struct_odds, pairs, mode, pairing="aligned", batch_records=BATCH_RECORDS):
    """``run`` with the records added up on the device (engine.expect_profile_merged)"""
    from . import _lib, occupancy, scanner, sites
    motif_ids = [sites.pair_id(a, b) for a, b in pairs]
    width = lambda a, b: (struct_odds[b] if b is not None else seq_odds[a]).length
    groups = occupancy._by_width([width(a, b) for a, b in pairs])
    with_seq, with_struct = pairs[0][0] is not None, pairs[0][1] is not None
    seq_tables = None
    if with_seq:
        seq_tables = dict((m, np.stack([seq_odds[pairs[k][0]].ratio_table(pack.RNA_LETTERS) for k in ks])) for m, ks in groups.items())
    folded = dict((m, _Folded(len(ks), m)) for m, ks in groups.items())
    acc_seq = dict((m, expect.new_acc(len(ks), m) if with_seq else None) for m, ks in groups.items())
    first = dict((m, (np.full((len(ks), 2), -1, dtype=np.int64), np.full((len(ks), 2), -1, dtype=np.int64))) for m, ks in groups.items())
    occs = dict((k, []) for k in range(len(pairs)))
    wins = dict((m, 0) for m in groups)                            # Windows depends on the width (and, with -p, on the codes)
    seen = []
    for a in range(0, len(profiles.ids), batch_records):
        b = min(len(profiles.ids), a + batch_records)
        at = a
        for ids, cols, pst in profiles.runs(a, b):
            stream = occupancy.paired_batch(recs, at, ids, pst)
            to_letters = [list(cols).index(l) for l in sites.STRUCT_ORDER]   # stored column of every letter of the written PFM
            for m, ks in groups.items():
                st = np.stack([scanner.struct_matrix(struct_odds[pairs[k][1]], cols, pairing) for k in ks]) if with_struct else None
                bs, bq, o, w = engine.expect_profile_merged(stream, st, seq_tables[m] if with_seq else None, mode,
                                                            folded[m].current(to_letters), acc_seq[m])
                expect.note_bad(first[m][0], np.asarray(bs), len(seen))
                if with_seq:
                    expect.note_bad(first[m][1], np.asarray(bq), len(seen))
                o = np.asarray(o)
                for j, k in enumerate(ks):
                    occs[k].append(o[:, j])
                wins[m] += int(np.asarray(w).sum())
            seen += list(ids)
            at += len(ids)
    place = dict((k, (m, j)) for m, ks in groups.items() for j, k in enumerate(ks))
    est = dict((m, _lib.site_acc_round(folded[m].fold()).reshape(len(ks), m, -1)[:, :, :7]) for m, ks in groups.items())
    esq = dict((m, _lib.site_acc_round(acc_seq[m]).reshape(len(ks), m, -1)[:, :, :4] if with_seq else None) for m, ks in groups.items())
    out = {}
    for k, mid in enumerate(motif_ids):
        if not occs[k]:
            raise expect.ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
        m, j = place[k]
        firsts, sums = [first[m][0][j]], [np.ascontiguousarray(est[m][j])]
        if with_seq:
            firsts.append(first[m][1][j])
            sums.append(np.ascontiguousarray(esq[m][j]))
        got = expect.merged_result(mid, np.concatenate(occs[k]), firsts, sums, seen, wins[m], NOT_FINITE)
        out[mid] = got if with_seq else (got[0], None) + got[1:]
    return out


def run_host(engine, recs, profiles, seq_odds, struct_odds, pairs, mode, pairing="aligned", batch_records=BATCH_RECORDS):
    """``run`` with every per-record matrix brought home and added up with math.fsum"""
    import math
    from . import occupancy, scanner, sites
    motif_ids = [sites.pair_id(a, b) for a, b in pairs]
    width = lambda a, b: (struct_odds[b] if b is not None else seq_odds[a]).length
    groups = occupancy._by_width([width(a, b) for a, b in pairs])
    with_seq, with_struct = pairs[0][0] is not None, pairs[0][1] is not None
    seq_tables = None
    if with_seq:
        seq_tables = dict((m, np.stack([seq_odds[pairs[k][0]].ratio_table(pack.RNA_LETTERS) for k in ks])) for m, ks in groups.items())
    est = dict((k, []) for k in range(len(pairs)))
    esq = dict((k, []) for k in range(len(pairs)))
    occs = dict((k, []) for k in range(len(pairs)))
    wins = dict((k, []) for k in range(len(pairs)))                # Windows depends on the width (and, with -p, on the codes)
    seen = []
    for a in range(0, len(profiles.ids), batch_records):
        b = min(len(profiles.ids), a + batch_records)
        at = a
        for ids, cols, pst in profiles.runs(a, b):
            stream = occupancy.paired_batch(recs, at, ids, pst)
            to_letters = [list(cols).index(l) for l in sites.STRUCT_ORDER]   # stored column of every letter of the written PFM
            for m, ks in groups.items():
                # the structure tables in THIS run's stored column order
                st = np.stack([scanner.struct_matrix(struct_odds[pairs[k][1]], cols, pairing) for k in ks]) if with_struct else None
                es, eq, o, w = engine.expect_profile(stream, st, seq_tables[m] if with_seq else None, mode)
                es, o = np.asarray(es), np.asarray(o)
                for j, k in enumerate(ks):
                    est[k].append(es[:, j][:, :, to_letters])
                    occs[k].append(o[:, j])
                    wins[k].append(np.asarray(w))
                    if with_seq:
                        esq[k].append(np.asarray(eq)[:, j, :, :4])
            seen += list(ids)
            at += len(ids)
    out = {}
    for k, mid in enumerate(motif_ids):
        if not occs[k]:
            raise expect.ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
        occ = np.concatenate(occs[k])
        bad = np.flatnonzero(~np.isfinite(occ))
        for cells in (est[k], esq[k]):
            if bad.size == 0 and cells:
                bad = np.flatnonzero(~np.isfinite(np.concatenate(cells, axis=0)).all(axis=(1, 2)))
        if bad.size:
            raise expect.ExpectError("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
                                     "(a ratio of the motif or a cell of the profile is; check the background and the pseudocount)" %
                                     (mid, seen[int(bad[0])]))
        counted = occ > 0
        if not counted.any():
            raise expect.ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
        ll = math.fsum(math.log2(x) for x in occ[counted].tolist())
        out[mid] = (expect.fsum_records(est[k]), expect.fsum_records(esq[k]) if with_seq else None, int(counted.sum()), int((~counted).sum()),
                    int(np.concatenate(wins[k]).sum()), round(ll, 3))
    return out


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.expect_profile",
                                     description=("Expected counts on averaged-structure profiles: the profile's rows (and the letters) "
                                                  "under every window, weighted by the window's likelihood ratio."))
    parser.add_argument("inputs", metavar="input", nargs="+",
                        help="the averaged-structure directory or packed store (-q alone); or the sequence FASTA and the directory or store (-p)")
    parser.add_argument("-p", "--pfm_seq", dest="pfm_seq", type=str, default=None, help="Sequence PFM")
    parser.add_argument("-q", "--pfm_struct", dest="pfm_struct", type=str, default=None, help="Structure PFM")
    parser.add_argument("-o", "--prefix", dest="prefix", type=str, required=True,
                        help="PREFIX of PREFIX.expected.struct.txt, PREFIX.expected.seq.txt and PREFIX.summary.txt")
    parser.add_argument("-C", "--pseudocount", type=float, dest="pseudocount", default=0, help="Pseudocount for normalizing PFM. [%(default)s]")
    parser.add_argument("-u", "--uniformbg", action="store_true", default=False, dest="uniform_background",
                        help="Use uniform background for the odds ratios [%(default)s]")
    parser.add_argument("-b", "--bg_seq", default=None, dest="bg_seq", help="File of pre-computed background probabilities for sequences")
    parser.add_argument("-B", "--bg_struct", default=None, dest="bg_struct", help="File of pre-computed background probabilities for structures")
    parser.add_argument("--weight", choices=sorted(expect.MODES), default="posterior",
                        help="weight of a window: its likelihood ratio, or that over the record's occupancy [%(default)s]")
    parser.add_argument("--iterations", type=int, default=1, help="passes: each takes the last one's expected matrices as its PFMs [%(default)s]")
    parser.add_argument("--all-motifs", action="store_true", default=False, dest="all_motifs", help="every motif (pair) of multi-PFM files, one call per width [off]")
    parser.add_argument("--pairing", choices=["aligned", "positional"], default="aligned",
                        help="averaged-structure columns vs structure PFM, as rnascan's [%(default)s]")
    parser.add_argument("--profile-dtype", choices=["float32", "float64"], default=None, dest="profile_dtype",
                        help="device storage of averaged-structure rows [the store's own dtype; float64 for text files]")
    parser.add_argument("--batch-records", type=int, default=BATCH_RECORDS, dest="batch_records",
                        help="records per device call; the files do not depend on it [%(default)s]")
    expect.add_merge_option(parser)
    parser.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")
    args = parser.parse_intermixed_args(argv)
    if args.uniform_background and (args.bg_seq or args.bg_struct):
        parser.error("You cannot set uniform and custom background options at the same time\n")
    if args.batch_records < 1:
        parser.error("--batch-records: must be positive")
    return args


def _check(args):
    """the option combinations, before anything is read -> message or None"""
    from . import occupancy
    if not args.pfm_seq and not args.pfm_struct:
        return "one of -p (sequence PFM) or -q (structure PFM), or both, is required"
    if args.iterations < 1:
        return "--iterations: must be at least 1, not %d" % args.iterations
    if args.iterations > 1 and args.pairing == "positional":
        return "--iterations %d with --pairing positional: the written columns are not the ones the PFM's letters were paired with" % args.iterations
    want = 2 if args.pfm_seq else 1
    if len(args.inputs) != want:
        return ("-p needs the sequence FASTA and the averaged-structure directory or packed store (seqs.fa avgdir/)" if args.pfm_seq else
                "-q alone takes one input, the averaged-structure directory or packed store")
    if not occupancy._is_profiles(args.inputs[-1]):
        return ("%s is not an averaged-structure directory or packed store: expected counts of a FASTA of letters are "
                "`python -m rnascan_amd.expect`" % args.inputs[-1])
    if args.pfm_seq and occupancy._is_profiles(args.inputs[0]):
        return "-p needs a sequence FASTA first, %s is an averaged-structure directory or store" % args.inputs[0]
    return None


def main(argv=None, engine=None):
    from . import background, occupancy, scanner, sites
    args = getoptions(argv)
    said = _check(args)
    if said:
        fasta.eprint(said)
        return 1
    own = engine is None
    struct_letters = list(sites.STRUCT_ORDER)
    try:
        motifs = occupancy.profile_motifs(args)
        if motifs is None:
            return 1
        pairs = motifs[0]
        if engine is None:
            engine = scanner.HipEngine(args.device)
        recs, profiles, seq_odds, struct_odds, bg_seq, bg_struct = occupancy.profile_sources(args, engine)
        motif_ids = [sites.pair_id(a, b) for a, b in pairs]
        summary = ["\t".join(expect.COLUMNS) + "\n"]
        got = None
        for it in range(1, args.iterations + 1):
            got = run(engine, recs, profiles, seq_odds, struct_odds, pairs, expect.MODES[args.weight], args.pairing, args.batch_records, args.merge)
            for mid in motif_ids:
                _, _, n, skipped, windows, ll = got[mid]
                summary.append("%s\t%d\t%d\t%d\t%d\t%s\n" % (mid, it, n, skipped, windows, repr(ll)))
            if it < args.iterations:
                # what reading this iteration's files would give: every motif (pair) under its written name
                if args.pfm_seq:
                    seq_odds = OrderedDict((mid, expect.next_odds(got[mid][1], fasta.RNA, pack.RNA_LETTERS, args.pseudocount, bg_seq)) for mid in motif_ids)
                if args.pfm_struct:
                    struct_odds = OrderedDict((mid, expect.next_odds(got[mid][0], fasta.STRUCT, struct_letters, args.pseudocount, bg_struct))
                                              for mid in motif_ids)
                pairs = [(mid if args.pfm_seq else None, mid if args.pfm_struct else None) for mid in motif_ids]
        texts = [(".expected.struct.txt", expect.pfm_text(dict((mid, got[mid][0]) for mid in motif_ids), motif_ids, sites.STRUCT_ORDER,
                                                          struct_letters, args.all_motifs))]
        if args.pfm_seq:
            texts.append((".expected.seq.txt", expect.pfm_text(dict((mid, got[mid][1]) for mid in motif_ids), motif_ids, sites.SEQ_ORDER,
                                                               pack.RNA_LETTERS, args.all_motifs)))
        for suffix, text in texts + [(".summary.txt", "".join(summary))]:
            with open(args.prefix + suffix, "w") as out:
                out.write(text)
        fasta.eprint("Wrote the expected counts of %d motifs after %d iterations" % (len(motif_ids), args.iterations))
        return 0
    except (IOError, expect.ExpectError, sites.InputError, background.BackgroundError, background.InputError) as e:
        fasta.eprint(str(e))
        return 1
    finally:
        if own and engine is not None:
            engine.close()


if __name__ == "__main__":
    sys.exit(main())
