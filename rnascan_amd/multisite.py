"""Multisite: the probability that a position is bound, under any number of non-overlapping sites per record -- none included.

    python -m rnascan_amd.multisite (-p seq.pfm | -q struct.pfm | -p seq.pfm -q struct.pfm) [-C c] [-u | -b bg | -B bg]
                                    [--prior-sites G | --lambda X] [--min-cover T] [--positions] [--records FILE]
                                    [--all-motifs] [--struct-format auto|letters|dotbracket] [--batch-records n] [--device d]
                                    in.fa [structs.fa] > regions.tsv

``footprint`` places exactly one site in every record, ``occupancy`` adds overlapping windows as if all were bound at once.
Here a record holds any set of non-overlapping sites: the weight of a set is the product of the activities
``a_s = ratio_s * lam`` of its sites, the empty set weighs 1, and the partition function ``Z`` is their sum.  The posterior that
a site starts at a window comes from a forward and a backward recurrence over the record, the cover of a position is the sum
of the posteriors of the at most m windows over it -- sites of one set do not overlap, so it is the probability that the
position is bound.  All of it is made on the GPU in rounded fp64 operations of a fixed order; only the positions whose cover is
greater than ``--min-cover`` come home, so the bytes written do not depend on ``--batch-records``.

``--prior-sites G`` (default 1.0) sets ``lam = G / max(L - m + 1, 1)`` per record and width: G sites expected a priori in a
record whose ratios are all 1.  ``--lambda X`` gives every record the same ``lam``.  Inputs are ``footprint``'s.

One row per region, as ``footprint`` writes them: Motif_ID Seq_ID Start End Peak.Pos Peak.Cover Mass, ``Mass`` the expected
number of sites that lie wholly inside the region.  ``--positions``: Motif_ID Seq_ID Pos Start.Weight Cover.  ``--records
FILE``: one row per record and motif, Motif_ID Seq_ID Windows Z Log2.Z P.Bound Expected.Sites with ``P.Bound = (Z - 1) / Z`` the
probability that the record holds a site at all.  Doubles are printed with ``repr``, Log2.Z rounded to 3 places.

There is no scaling: ``Z`` grows like ``exp(lam * sum of ratios)`` and overflows on long records with a large prior.  An infinite
or NaN ``Z`` is an error that names the motif and the record, and nothing is written.

Not supported: averaged-structure directories or stores (they are ``python -m rnascan_amd.multisite_profile``), expected counts
or mutagenesis under this model, cooperativity or spacing between sites, a scaled recurrence for records whose Z overflows,
``--gpus``, bedGraph output.
"""
import argparse
import math
import sys

import numpy as np

from . import fasta, footprint, occupancy, occupancy_pair

COLUMNS, POSITION_COLUMNS = footprint.COLUMNS, footprint.POSITION_COLUMNS
RECORD_COLUMNS = ["Motif_ID", "Seq_ID", "Windows", "Z", "Log2.Z", "P.Bound", "Expected.Sites"]
NOT_FINITE = ("Motif %s, record %s: the partition function Z is infinite or not a number (the record is too long for this prior, or a "
              "ratio of the motif is not finite); give a smaller --prior-sites or --lambda")
NO_PROFILES = ("%s is an averaged-structure directory or packed store: the multi-site model takes FASTA files of letters "
               "(averaged-structure profiles are not supported by this command)")


class MultisiteError(ValueError):
    """what the pass found: said on stderr, exit 1, nothing written"""


def lam_of(lengths, m, prior_sites, lam):
    """the activity of a site per record: ``lam`` for all, or prior_sites / max(L - m + 1, 1), one division per record"""
    lengths = np.asarray(lengths, dtype=np.int64)
    if lam is not None:
        return np.full(lengths.size, float(lam), dtype=np.float64)
    return np.float64(prior_sites) / np.maximum(lengths - m + 1, 1).astype(np.float64)


def record_rows(motif_ids, ids, win, z, nsites):
    """the lines of --records for one batch, (record, motif) order"""
    lines = []
    for r, sid in enumerate(ids):
        for k, mid in enumerate(motif_ids):
            zz = float(z[r, k])
            lines.append("%s\t%s\t%d\t%s\t%s\t%s\t%s\n" % (mid, sid, int(win[r, k]), repr(zz), occupancy.log2_text(zz), repr((zz - 1.0) / zz),
                                                         repr(float(nsites[r, k]))))
    return lines


def batch_rows(motif_ids, groups, ids, stream, call, positions, cols=None, not_positive=None):
    """the lines of one batch in (record, motif, position) order and its --records lines.
    ``call(stream, m, ks)`` -> (key, cover, start, z [n_rec][len(ks)], nsites, windows [n_rec]); a batch of averaged-structure
    profiles comes with its stored column order and is ``call(stream, m, ks, cols)``.  ``not_positive``: the message (motif,
    record) for a Z <= 0.0, which only negative profile cells can make; None: not tested"""
    n_pos = int(np.asarray(stream.codes).size) if stream.codes is not None else int(np.asarray(stream.profile).shape[0])
    offsets = np.asarray(stream.offsets, dtype=np.int64)
    got = {}                                                       # (record, motif) -> (positions in the record, cover, start, width)
    z = np.ones((len(ids), len(motif_ids)), dtype=np.float64)
    ns = np.zeros((len(ids), len(motif_ids)), dtype=np.float64)
    win = np.zeros((len(ids), len(motif_ids)), dtype=np.int64)
    for m, ks in groups.items():
        key, cover, start, zz, nn, w = call(stream, m, ks) if cols is None else call(stream, m, ks, cols)
        z[:, ks], ns[:, ks] = np.asarray(zz), np.asarray(nn)
        win[:, ks] = np.asarray(w)[:, None]
        key = np.asarray(key, dtype=np.int64)
        j, p = key // max(n_pos, 1), key % max(n_pos, 1)
        r = np.searchsorted(offsets, p, side="right") - 1
        # the keys are sorted: motif, then position, so the events of a (motif, record) are a run
        cut = np.flatnonzero((np.diff(j) != 0) | (np.diff(r) != 0)) + 1 if key.size else np.zeros(0, dtype=np.int64)
        for a, b in zip(np.concatenate([[0], cut]).astype(int), np.concatenate([cut, [key.size]]).astype(int)):
            if b > a:
                got[(int(r[a]), ks[int(j[a])])] = (p[a:b] - offsets[r[a]], cover[a:b], start[a:b], m)
    bad = np.argwhere(~np.isfinite(z))
    if bad.size:
        raise MultisiteError(NOT_FINITE % (motif_ids[int(bad[0][1])], ids[int(bad[0][0])]))
    if not_positive:
        bad = np.argwhere(z <= 0.0)
        if bad.size:
            raise MultisiteError(not_positive % (motif_ids[int(bad[0][1])], ids[int(bad[0][0])]))
    lines = []
    for r, sid in enumerate(ids):
        for k, mid in enumerate(motif_ids):
            if (r, k) in got:
                pos, cover, start, m = got[(r, k)]
                lines += footprint.format_rows(mid, sid, pos, cover, start, m, positions)
    return lines, record_rows(motif_ids, ids, win, z, ns)


def write_table(out, records_path, motif_ids, groups, batches, call, positions, not_positive=None):
    """every line is made before the first is written: a record that fails leaves nothing behind"""
    lines, rec_lines = [], []
    for ids, stream, cols in batches:
        more, recs = batch_rows(motif_ids, groups, ids, stream, call, positions, cols, not_positive)
        lines += more
        rec_lines += recs
    out.write("\t".join(POSITION_COLUMNS if positions else COLUMNS) + "\n")
    out.write("".join(lines))
    out.flush()
    if records_path:
        with open(records_path, "w") as f:
            f.write("\t".join(RECORD_COLUMNS) + "\n")
            f.write("".join(rec_lines))
    fasta.eprint("Wrote %d rows" % len(lines))


OPTIONS = dict(occupancy.OPTIONS)
OPTIONS.update({
    "--prior-sites": lambda p, w: p.add_argument("--prior-sites", type=float, default=None, dest="prior_sites", metavar="G",
                                                 help="sites expected a priori per record: lam = G / max(L - m + 1, 1) [1.0]"),
    "--lambda": lambda p, w: p.add_argument("--lambda", type=float, default=None, dest="lam", metavar="X",
                                            help="the same activity lam for every record instead of --prior-sites"),
    "--min-cover": lambda p, w: p.add_argument("--min-cover", type=float, default=0.5, dest="min_cover", metavar="T",
                                               help="report the positions whose probability of being bound is greater than T [%(default)s]"),
    "--positions": footprint.OPTIONS["--positions"],
    "--records": lambda p, w: p.add_argument("--records", type=str, default=None, dest="records", metavar="FILE",
                                             help="also write the per-record table (Z, P.Bound, Expected.Sites) to FILE"),
})


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.multisite",
                                     description=("Multisite: the probability that a position is bound under any number of non-overlapping "
                                                  "sites per record, reported as the regions (or positions) whose cover passes --min-cover."))
    parser.add_argument("inputs", metavar="input", nargs="+",
                        help="the sequence FASTA (-p) or structure FASTA (-q); or both, sequences first (-p with -q)")
    occupancy.add_options(parser, ["-p", "-q", "-C", "-u", "-b", "-B", "--prior-sites", "--lambda", "--min-cover", "--positions", "--records",
                                   "--all-motifs", "--struct-format", "--batch-records", "--device"], OPTIONS,
                          every="motif (or pair) of multi-PFM files", q="", result="output does", joint="")
    args = parser.parse_intermixed_args(argv)
    occupancy.check_options(parser, args)
    if args.prior_sites is not None and args.lam is not None:
        parser.error("--prior-sites and --lambda are mutually exclusive")
    for name, x in (("--prior-sites", args.prior_sites), ("--lambda", args.lam)):
        if x is not None and not (math.isfinite(x) and x >= 0.0):
            parser.error("%s: must be finite and >= 0" % name)
    if args.prior_sites is None and args.lam is None:
        args.prior_sites = 1.0
    if args.min_cover != args.min_cover:
        parser.error("--min-cover: not a number")
    args.single, args.profiles = "multisite", "occupancy"
    args.fasta = args.inputs[0]
    return args


def main(argv=None, engine=None, out=None):
    from . import sites
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    if not args.pfm_seq and not args.pfm_struct:
        fasta.eprint("one of -p (sequence PFM) or -q (structure PFM), or both, is required")
        return 1
    pair = bool(args.pfm_seq) and bool(args.pfm_struct)
    for path in args.inputs:
        if occupancy._is_profiles(path):
            fasta.eprint(NO_PROFILES % path)
            return 1
    if pair:
        checked = occupancy_pair.check_inputs(args)
        if checked is None:
            return 1
    elif len(args.inputs) != 1:
        fasta.eprint("%s alone takes one input: give -p and -q with the sequence FASTA and the structure FASTA" % ("-p" if args.pfm_seq else "-q"))
        return 1
    with occupancy.Device(engine, args.device, (IOError, sites.InputError, MultisiteError)) as dev:
        if pair:
            pairs = checked[0]
            engine = dev.engine
            recs, srecs, seq_odds, struct_odds, _, _ = occupancy_pair.sources(args, engine)
            motif_ids = [sites.pair_id(a, b) for a, b in pairs]
            groups = occupancy._by_width([seq_odds[a].length for a, _ in pairs])
            tables = dict((m, occupancy_pair.pair_tables(seq_odds, struct_odds, pairs, ks)) for m, ks in groups.items())
            batches = occupancy_pair.batches(recs, srecs, args.batch_records)
        else:
            got = occupancy.single_fasta(args, dev)
            if got is None:
                return 1
            motif_ids, letters, code_letters, _, odds, recs = got
            engine = dev.engine
            groups = occupancy._by_width([odds[mid].length for mid in motif_ids])
            stacks = dict((m, np.stack([odds[motif_ids[k]].ratio_table(code_letters) for k in ks])) for m, ks in groups.items())
            tables = dict((m, (t, None) if args.pfm_seq else (None, t)) for m, t in stacks.items())
            batches = occupancy.letter_batches(recs, letters, args.batch_records)
        write_table(out, args.records, motif_ids, groups, batches,
                    lambda stream, m, ks: engine.multisite_events(stream, tables[m][0], tables[m][1],
                                                                  lam_of(stream.lengths, m, args.prior_sites, args.lam), args.min_cover),
                    args.positions)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
