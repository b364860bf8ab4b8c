"""Footprint on averaged-structure profiles: where in each record does the motif bind, without a threshold on the score.

    python -m rnascan_amd.footprint_profile -q struct.pfm [...] avgdir_or_store/ > regions.tsv
    python -m rnascan_amd.footprint_profile -p seq.pfm -q struct.pfm [...] seqs.fa avgdir_or_store/ > regions.tsv
        [-C c] [-u | -b bg | -B bg] [--weight posterior|ratio] [--min-cover T] [--positions] [--all-motifs]
        [--pairing aligned|positional] [--profile-dtype float32|float64] [--batch-records n] [--device d]

``footprint`` for the project's main input.  Every window of a record is weighted as ``expect_profile`` weights it: by the
structure motif's marginal ratios over the rows of the averaged-structure profile (``-q`` alone) or by their product with the
sequence motif's ratios over the FASTA's letters, the ratio behind ``LogOdds.SeqStruct`` (``-p`` with ``-q``); the weight is
that ratio (``--weight ratio``) or the ratio over the record's occupancy (``--weight posterior``, the default).  The cover of a
position is the sum of the weights of the at most m windows over it, added in ascending order of their starts.
The weights and the covers are made on the GPU, and only the positions whose cover is greater than ``--min-cover`` come home,
so the bytes written do not depend on ``--batch-records``.

Records and profiles are matched by id, two libraries are paired, widths are checked, the structure background defaults to
the profiles' own, and the rows' storage and the runs of equal stored column order are chosen exactly as ``occupancy`` does it
(the same code).  The rows, the columns, ``--min-cover`` (0.5 with posterior weights, required with ``--weight ratio``), the
``repr`` doubles, the count of records with occupancy 0 on stderr and the error for an infinite or NaN occupancy are
``footprint``'s (the same code).  Profile cells may be negative (``-u`` / ``-B``): an occupancy can then be negative, and its
record's rows are what the arithmetic gives.

Not supported: ``-p`` alone (sequence weights are ``python -m rnascan_amd.footprint`` on the FASTA), ``--gpus``, bedGraph or
bigWig output, merging regions on the device, more or fewer than one site per record (ZOOPS), ``--flank``.
"""
import argparse
import sys

from . import fasta, footprint, occupancy

MODES = footprint.MODES


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.footprint_profile",
                                     description=("Footprint on averaged-structure profiles: the posterior site coverage of every position, "
                                                  "reported as the regions (or positions) whose cover passes --min-cover."))
    parser.add_argument("inputs", metavar="input", nargs="+",
                        help="the averaged-structure directory or packed store (-q alone); or the sequence FASTA and the directory or store (-p with -q)")
    occupancy.add_options(parser, ["-p", "-q", "-C", "-u", "-b", "-B", "--weight", "--min-cover", "--positions", "--all-motifs", "--pairing",
                                   "--profile-dtype", "--batch-records", "--device"], footprint.OPTIONS, every="motif (or pair) of multi-PFM files",
                          result="output does", joint="")
    args = parser.parse_intermixed_args(argv)
    occupancy.check_options(parser, args)
    if args.min_cover is None:
        if args.weight != "posterior":
            parser.error("--min-cover is required with --weight ratio: likelihood ratios have no natural scale")
        args.min_cover = 0.5
    if args.min_cover != args.min_cover:
        parser.error("--min-cover: not a number")
    return args


def _check(args):
    """the option combinations, before anything is read -> message or None"""
    if not args.pfm_struct:
        return ("-q (structure PFM) is required, alone or with -p: the sequence weights of a FASTA are `python -m rnascan_amd.footprint -p`"
                if args.pfm_seq else "-q (structure PFM), or -p with -q, is required")
    want = 2 if args.pfm_seq else 1
    if len(args.inputs) != want:
        return ("-p with -q needs the sequence FASTA and the averaged-structure directory or packed store (seqs.fa avgdir/)" if args.pfm_seq else
                "-q alone takes one input, the averaged-structure directory or packed store")
    if not occupancy._is_profiles(args.inputs[-1]):
        return ("%s is not an averaged-structure directory or packed store: the footprint of a FASTA of letters is "
                "`python -m rnascan_amd.footprint`" % args.inputs[-1])
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
    mode = MODES[args.weight]
    with occupancy.Device(engine, args.device, (IOError, sites.InputError, background.BackgroundError, background.InputError,
                                                footprint.FootprintError)) as dev:
        motifs = occupancy.profile_motifs(args)
        if motifs is None:
            return 1
        pairs = motifs[0]
        engine = dev.engine
        recs, profiles, seq_odds, struct_odds, _, _ = occupancy.profile_sources(args, engine)
        groups = occupancy._by_width([struct_odds[b].length for _, b in pairs])
        tables = occupancy.profile_tables(seq_odds, struct_odds, pairs, args.pairing)
        footprint.write_table(out, [sites.pair_id(a, b) for a, b in pairs], groups, occupancy.profile_batches(recs, profiles, args.batch_records),
                              lambda stream, m, ks, cols: engine.footprint_profile_events(stream, *tables(m, ks, cols), mode, args.min_cover),
                              args.positions)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
