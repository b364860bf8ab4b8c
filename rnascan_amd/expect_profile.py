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
import sys

from . import expect, fasta, occupancy, pack

BATCH_RECORDS = expect.BATCH_RECORDS
NOT_FINITE = ("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
              "(a ratio of the motif or a cell of the profile is; check the background and the pseudocount)")


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.expect_profile",
                                     description=("Expected counts on averaged-structure profiles: the profile's rows (and the letters) "
                                                  "under every window, weighted by the window's likelihood ratio."))
    parser.add_argument("inputs", metavar="input", nargs="+",
                        help="the averaged-structure directory or packed store (-q alone); or the sequence FASTA and the directory or store (-p)")
    occupancy.add_options(parser, ["-p", "-q", "-o", "-C", "-u", "-b", "-B", "--weight", "--iterations", "--all-motifs", "--pairing", "--profile-dtype",
                                   "--batch-records", "--merge", "--device"], expect.OPTIONS, every="motif (pair) of multi-PFM files",
                          result="files do", joint="", files="PREFIX.expected.struct.txt, PREFIX.expected.seq.txt and PREFIX.summary.txt",
                          steps="passes: each takes the last one's expected matrices as its PFMs")
    args = parser.parse_intermixed_args(argv)
    occupancy.check_options(parser, args)
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
    from . import background, sites
    args = getoptions(argv)
    said = _check(args)
    if said:
        fasta.eprint(said)
        return 1
    with occupancy.Device(engine, args.device, (IOError, expect.ExpectError, sites.InputError, background.BackgroundError, background.InputError)) as dev:
        motifs = occupancy.profile_motifs(args)
        if motifs is None:
            return 1
        engine = dev.engine
        recs, profiles, seq_odds, struct_odds, bg_seq, bg_struct = occupancy.profile_sources(args, engine)

        def form_of(odds, pairs):
            """one pass -> per motif (pair) (E_struct [m][7] in sites.STRUCT_ORDER, then with -p E_seq [m][4] in code order).  The
            weights come from the sequence tables, the structure tables or both; the profile's rows are always added up"""
            with_seq = pairs[0][0] is not None
            width = lambda a, b: (odds[1][b] if b is not None else odds[0][a]).length

            def host(stream, tables, mode):
                es, eq, o, w = engine.expect_profile(stream, tables[0], tables[1], mode)
                return [es, eq], o, w

            def merged(stream, tables, mode, accs):
                bs, bq, o, w = engine.expect_profile_merged(stream, tables[0], tables[1], mode, accs[0], accs[1] if with_seq else None)
                return [bs, bq], o, w
            # the structure matrix comes in the run's stored column order: the stored column of every letter of the written PFM
            stored = lambda cols: [list(cols).index(l) for l in sites.STRUCT_ORDER]
            return expect.Form([sites.pair_id(a, b) for a, b in pairs], occupancy._by_width([width(a, b) for a, b in pairs]), range(len(pairs)),
                               lambda: occupancy.profile_batches(recs, profiles, args.batch_records),
                               occupancy.profile_tables(odds[0], odds[1], pairs, args.pairing), host, merged, "expect_profile_merged",
                               [expect.Matrix(7, stored)] + [expect.Matrix(4)] * with_seq, NOT_FINITE)

        sides = [expect.Side(".expected.struct.txt", 1, list(sites.STRUCT_ORDER), bg_struct)]
        if args.pfm_seq:
            sides.append(expect.Side(".expected.seq.txt", 0, pack.RNA_LETTERS, bg_seq))
        expect.iterate(args, engine, sides, [seq_odds, struct_odds], motifs[0], form_of)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
