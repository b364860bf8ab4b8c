"""Multisite on averaged-structure profiles: the probability that a position is bound, under any number of non-overlapping sites.

    python -m rnascan_amd.multisite_profile -q struct.pfm [...] avgdir_or_store/ > regions.tsv
    python -m rnascan_amd.multisite_profile -p seq.pfm -q struct.pfm [...] seqs.fa avgdir_or_store/ > regions.tsv
        [-C c] [-u | -b bg | -B bg] [--prior-sites G | --lambda X] [--min-cover T] [--positions] [--records FILE]
        [--all-motifs] [--pairing aligned|positional] [--profile-dtype float32|float64] [--batch-records n] [--device d]

``multisite`` for the project's main input (DESIGN.md 5n "on averaged-structure profiles").  The ratio of a window is the one
``occupancy``, ``expect_profile`` and ``footprint_profile`` use on profiles: the structure motif's marginal ratios over the rows
of the averaged-structure profile (``-q`` alone) or their product with the sequence motif's ratios over the FASTA's letters, the
ratio behind ``LogOdds.SeqStruct`` (``-p`` with ``-q``).  The activities ``a_s = ratio_s * lam``, the partition function ``Z``
over every set of non-overlapping sites, the posterior that a site starts at a window, the cover of a position and the
expected number of sites are ``multisite``'s, made on the GPU by the same kernels; only the positions whose cover is greater
than ``--min-cover`` come home, so the bytes written do not depend on ``--batch-records``, nor on whether the profiles come
from a directory or a packed store.  They do depend on the rows' storage (``--profile-dtype``) and the stored column order.

Records and profiles are matched by id, two libraries are paired, widths are checked, the structure background defaults to
the profiles' own, and the rows' storage and the runs of equal stored column order are chosen exactly as ``footprint_profile``
does it (the same code).  ``--prior-sites``, ``--lambda``, ``--min-cover`` (default 0.5), ``--positions``, ``--records``, the
rows, the columns and the ``repr`` doubles are ``multisite``'s (the same code).

There is no scaling: an infinite or NaN ``Z`` is an error that names the motif and the record, and nothing is written.  With
near-one-hot rows and a small pseudocount the marginal ratios are large, and ``Z`` is far nearer that overflow than on letters.
Profile cells may be negative (``-u`` / ``-B``).  Where they drive ``Z`` to zero or below, ``Log2.Z`` and ``P.Bound`` mean
nothing: that too is an error that names the motif and the record and says so, and nothing is written.  Negative cells that
leave ``Z`` positive print what the arithmetic gives: a start weight or a cover can then be negative or greater than 1.

Not supported: ``-p`` alone (the model of a FASTA's letters is ``python -m rnascan_amd.multisite``), a scaled or log-space
recurrence, expected counts or mutagenesis under this model, ``--gpus``, ``--flank``, bedGraph output.
"""
import argparse
import math
import sys

from . import fasta, multisite, occupancy

NOT_POSITIVE = ("Motif %s, record %s: the partition function Z is zero or negative (only negative profile cells can make it so, -u or a "
                "background larger than the profile's cells); Log2.Z and P.Bound mean nothing then")


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.multisite_profile",
                                     description=("Multisite on averaged-structure profiles: the probability that a position is bound under any "
                                                  "number of non-overlapping sites per record, reported as the regions (or positions) whose "
                                                  "cover passes --min-cover."))
    parser.add_argument("inputs", metavar="input", nargs="+",
                        help="the averaged-structure directory or packed store (-q alone); or the sequence FASTA and the directory or store (-p with -q)")
    occupancy.add_options(parser, ["-p", "-q", "-C", "-u", "-b", "-B", "--prior-sites", "--lambda", "--min-cover", "--positions", "--records",
                                   "--all-motifs", "--pairing", "--profile-dtype", "--batch-records", "--device"], multisite.OPTIONS,
                          every="motif (or pair) of multi-PFM files", result="output does", joint="")
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
    return args


def _check(args):
    """the option combinations, before anything is read -> message or None"""
    if not args.pfm_struct:
        return ("-q (structure PFM) is required, alone or with -p: the multi-site model of a FASTA's letters is `python -m rnascan_amd.multisite -p`"
                if args.pfm_seq else "-q (structure PFM), or -p with -q, is required")
    want = 2 if args.pfm_seq else 1
    if len(args.inputs) != want:
        return ("-p with -q needs the sequence FASTA and the averaged-structure directory or packed store (seqs.fa avgdir/)" if args.pfm_seq else
                "-q alone takes one input, the averaged-structure directory or packed store")
    if not occupancy._is_profiles(args.inputs[-1]):
        return ("%s is not an averaged-structure directory or packed store: the multi-site model of a FASTA of letters is "
                "`python -m rnascan_amd.multisite`" % args.inputs[-1])
    if args.pfm_seq and occupancy._is_profiles(args.inputs[0]):
        return "-p needs a sequence FASTA first, %s is an averaged-structure directory or store" % args.inputs[0]
    return None


def main(argv=None, engine=None, out=None):
    from . import background, sites
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    said = _check(args)
    if said:
        fasta.eprint(said)
        return 1
    with occupancy.Device(engine, args.device, (IOError, sites.InputError, background.BackgroundError, background.InputError,
                                                multisite.MultisiteError)) as dev:
        motifs = occupancy.profile_motifs(args)
        if motifs is None:
            return 1
        pairs = motifs[0]
        engine = dev.engine
        recs, profiles, seq_odds, struct_odds, _, _ = occupancy.profile_sources(args, engine)
        groups = occupancy._by_width([struct_odds[b].length for _, b in pairs])
        tables = occupancy.profile_tables(seq_odds, struct_odds, pairs, args.pairing)
        multisite.write_table(out, args.records, [sites.pair_id(a, b) for a, b in pairs], groups,
                              occupancy.profile_batches(recs, profiles, args.batch_records),
                              lambda stream, m, ks, cols: engine.multisite_profile_events(
                                  stream, *tables(m, ks, cols), multisite.lam_of(stream.lengths, m, args.prior_sites, args.lam), args.min_cover),
                              args.positions, NOT_POSITIVE)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
