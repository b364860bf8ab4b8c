"""Expected counts on averaged-structure profiles: the structural context of a motif's sites, without a threshold.

    python -m rnascan_amd.expect_profile -q struct.pfm [...] avgdir_or_store/ -o PREFIX
    python -m rnascan_amd.expect_profile -p seq.pfm -q struct.pfm [...] seqs.fa avgdir_or_store/ -o PREFIX
    python -m rnascan_amd.expect_profile -p seq.pfm [...] seqs.fa avgdir_or_store/ -o PREFIX
        [-C c] [-u | -b bg | -B bg] [--weight posterior|ratio] [--iterations N] [--joint] [--all-motifs]
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

``--joint`` (needs ``-p``: the table reads the sequences) also writes ``PREFIX.expected.joint.txt``: per motif column the
expected amount of structural context ``c`` under nucleotide ``a``, ``E[k][a][c]`` = the sum over the windows whose letter under
column ``k`` is ``a`` of ``w * r[s + k][c]`` -- the 4 x 7 table whose margins the two matrices are (to rounding), in the format of
``expect_pair --joint`` and of ``sites``' ``PREFIX.joint.txt``: ``PO``, the 28 cells ``A.B A.E ... U.T`` and ``MI``, the column's
mutual information in bits (``nan`` for a column with a negative cell, which is no distribution), one block per motif (pair)
tagged with a leading ``Motif`` column with ``--all-motifs``.  The table is summed on the GPU by the same rules,
goes through the same merge and the same checks as the two matrices (checked in the order structure, sequence, table), and
leaves the other files as they are.  On the device the per-record table is four times a matrix (32 doubles per record, motif
and column); ``--batch-records`` bounds it.

``--iterations N``: every given PFM is replaced by its own expected matrix, normalised with the same pseudocount against the
same background, and the pass is run again; with ``-p`` alone the sequence matrix is fed back and the structure matrix is
the last pass's.  ``--iterations 2`` writes the bytes of a run on the outputs of a run.  Refused with ``--pairing
positional``, under which the written columns are not the ones the PFM's letters were paired with.  The table of ``--joint`` is
the last pass's and is not fed back.

Not supported: ``--flank``, ``--joint`` with ``-q`` alone, two-FASTA pairs, ``--gpus``, other priors.
"""
import argparse
import math
import sys

import numpy as np

from . import expect, expect_pair, fasta, occupancy, pack

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
    parser.add_argument("--joint", action="store_true", default=False,
                        help="with -p: also write PREFIX.expected.joint.txt, per column the expected 4 x 7 table of structural context "
                             "under every nucleotide (the two matrices are its margins) and its mutual information; the per-record table "
                             "takes four times a matrix's device memory, which --batch-records bounds [off]")
    args = parser.parse_intermixed_args(argv)
    occupancy.check_options(parser, args)
    return args


def mutual_information(cells):
    """``expect_pair.mutual_information``; nan for a column with a negative cell (negative profile cells under -u / -B): no distribution"""
    if any(c < 0 for row in cells for c in row):
        return math.nan
    return expect_pair.mutual_information(cells)


def _check(args):
    """the option combinations, before anything is read -> message or None"""
    from . import occupancy
    if not args.pfm_seq and not args.pfm_struct:
        return "one of -p (sequence PFM) or -q (structure PFM), or both, is required"
    if args.joint and not args.pfm_seq:
        return "--joint needs -p: the table counts the profile's rows under every nucleotide, which it reads from the sequences"
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
                if args.joint:
                    es, eq, ej, o, w = engine.expect_profile_joint(stream, tables[0], tables[1], mode)
                    ej = np.asarray(ej)
                    return [es, eq, ej.reshape(ej.shape[:2] + (-1, ej.shape[-1]))], o, w
                es, eq, o, w = engine.expect_profile(stream, tables[0], tables[1], mode)
                return [es, eq], o, w

            def merged(stream, tables, mode, accs):
                if args.joint:
                    bs, bq, bj, o, w = engine.expect_profile_joint_merged(stream, tables[0], tables[1], mode, accs[0], accs[1], accs[2])
                    return [bs, bq, bj], o, w
                bs, bq, o, w = engine.expect_profile_merged(stream, tables[0], tables[1], mode, accs[0], accs[1] if with_seq else None)
                return [bs, bq], o, w
            # the structure matrix comes in the run's stored column order: the stored column of every letter of the written PFM
            stored = lambda cols: [list(cols).index(l) for l in sites.STRUCT_ORDER]
            # the table's 7 columns too; it is written by the code of sites' joint file, which takes them in code order
            coded = lambda cols: [list(cols).index(l) for l in pack.STRUCT_LETTERS]
            return expect.Form([sites.pair_id(a, b) for a, b in pairs], occupancy._by_width([width(a, b) for a, b in pairs]), range(len(pairs)),
                               lambda: occupancy.profile_batches(recs, profiles, args.batch_records),
                               occupancy.profile_tables(odds[0], odds[1], pairs, args.pairing), host, merged,
                               "expect_profile_joint_merged" if args.joint else "expect_profile_merged",
                               [expect.Matrix(7, stored)] + [expect.Matrix(4)] * with_seq + [expect.Matrix(7, coded, 4)] * args.joint, NOT_FINITE)

        def more(matrices, motif_ids):
            text = expect_pair.joint_text(dict((mid, matrices[mid][2]) for mid in motif_ids), motif_ids, args.all_motifs, mutual_information)
            # the table writer leaves a field that is not a number empty: MI, the last one, is written as nan
            return [(".expected.joint.txt", "".join(ln[:-1] + "nan\n" if ln.endswith("\t\n") else ln for ln in text.splitlines(True)))]

        sides = [expect.Side(".expected.struct.txt", 1, list(sites.STRUCT_ORDER), bg_struct)]
        if args.pfm_seq:
            sides.append(expect.Side(".expected.seq.txt", 0, pack.RNA_LETTERS, bg_seq))
        expect.iterate(args, engine, sides, [seq_odds, struct_odds], motifs[0], form_of, more=more if args.joint else None)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
