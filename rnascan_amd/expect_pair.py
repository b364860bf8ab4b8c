"""Expected site counts of sequence + structure FASTA pairs: one EM step (or several) on both motifs of a pair at once.

    python -m rnascan_amd.expect_pair -p seq.pfm -q struct.pfm [-C c] [-u | -b bg -B bg] [--weight posterior|ratio]
                                      [--iterations N] [--joint] [--all-motifs] [--struct-format auto|letters|dotbracket]
                                      [--batch-records n] [--merge auto|device|host] [--device d] -o PREFIX seqs.fa structs.fa

Every window of every record is weighted by its JOINT likelihood ratio -- the sequence ratio times the structure ratio, the
ratio behind ``LogOdds.SeqStruct`` (``--weight ratio``) -- or by that over the record's joint occupancy (``--weight
posterior``, the default: one site per record in expectation).  Under these weights the letters of BOTH files are added up:
``E_seq[k][c]`` is the expected number of times nucleotide ``c`` lies under motif column ``k``, ``E_struct[k][c]`` the same
for structure letter ``c``.  The joint weight of a window cannot be recovered from ``expect -p`` and ``expect -q``.  Weights
and per-record sums are made on the GPU by the rules of DESIGN.md 5j; the records are added up exactly, on the device or with
``math.fsum`` on the host (``--merge``, DESIGN.md 5k: the same bytes), so the bytes written do not depend on
``--batch-records`` or on the order of the records.

``PREFIX.expected.seq.txt`` is a raw-sum PFM that ``-p`` reads, ``PREFIX.expected.struct.txt`` one that ``-q`` reads -- the
names and formats of ``expect_profile``: multi-PFM libraries in pair order with ``--all-motifs`` (pairs named as the site
profiles name them), the first pair otherwise.  ``PREFIX.summary.txt`` has ``expect``'s columns.

``--joint`` also writes ``PREFIX.expected.joint.txt``: per motif column the expected number of times nucleotide ``a`` lies
OVER structure letter ``b`` under the same weights -- the 4 x 7 table whose margins the two matrices are, and the threshold-free
sibling of ``sites``' ``PREFIX.joint.txt``: ``PO``, the 28 cells under that file's column names (``A.B A.E ... U.T``) and ``MI``,
the column's mutual information in bits, one block per pair tagged with a leading ``Motif`` column with ``--all-motifs``.  Every
cell is written in the shortest form that reads back to the same double; the table is summed on the GPU by the same rules, goes
through the same merge and the same checks as the two matrices, and leaves the other files as they are.  On the device the
per-record table is four times a matrix (32 doubles per record, pair and column: 3.2 GB for 4096 records x 256 pairs of width
12); ``--batch-records`` bounds it.

``--iterations N``: both PFMs of a pair are replaced by their expected matrices, normalised with the same pseudocount
against the same backgrounds, and the pass is run again; ``--iterations 2`` writes the bytes of a run on the outputs of a run.
The table is the last pass's and is not fed back: its margins are.

Inputs, pairing, backgrounds and dot-bracket structures are handled exactly as ``occupancy_pair`` handles them (the same
code).  Not supported: a joint table with flanks, ``--gpus``, other priors.  (Averaged-structure profiles have their own table:
``expect_profile --joint``.)
"""
import argparse
import io
import math
import sys

import numpy as np

from . import expect, fasta, occupancy, occupancy_pair, pack

BATCH_RECORDS = expect.BATCH_RECORDS
NOT_FINITE = ("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
              "(a ratio of one of the motifs is; check the backgrounds and the pseudocount)")


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.expect_pair",
                                     description=("Expected site counts of sequence + structure FASTA pairs: the letters of both files "
                                                  "under every window, weighted by the window's joint likelihood ratio."))
    occupancy_pair.add_options(parser, expect.OPTIONS)
    occupancy.add_options(parser, ["-o", "--weight", "--iterations", "--merge"], expect.OPTIONS, joint="joint ",
                          files="PREFIX.expected.seq.txt, PREFIX.expected.struct.txt and PREFIX.summary.txt",
                          steps="EM steps: each takes the last one's expected matrices as its PFMs")
    parser.add_argument("--joint", action="store_true", default=False,
                        help="also write PREFIX.expected.joint.txt: per column the expected 4 x 7 table of nucleotide over structure letter "
                             "(the two matrices are its margins) and its mutual information; the per-record table takes four times a "
                             "matrix's device memory, which --batch-records bounds [off]")
    args = parser.parse_intermixed_args(argv)
    occupancy.check_options(parser, args)
    args.single, args.profiles = "expect", "expect_profile"
    return args


def mutual_information(cells):
    """``sites.mutual_information`` on expected counts (floats): the total and the margins are taken with math.fsum"""
    total = math.fsum(c for row in cells for c in row)
    if total == 0:
        return 0.0
    pa = [math.fsum(row) / total for row in cells]
    pb = [math.fsum(row[b] for row in cells) / total for b in range(len(cells[0]))]
    return math.fsum((c / total) * math.log2((c / total) / (pa[a] * pb[b]))
                     for a, row in enumerate(cells) for b, c in enumerate(row) if c)


def joint_text(tables, motif_ids, library, mi=mutual_information):
    """PREFIX.expected.joint.txt from {pair id: E_joint float64 [4 m][7], row k * 4 + a, both letters in code order}: ``sites``'
    PREFIX.joint.txt with expected counts in the cells, written and (with ``library``) tagged by the same code; ``mi``: the
    mutual information of a column's cells (``expect_profile --joint`` has its own for negative cells)"""
    from . import sites
    text = io.StringIO()
    for mid in motif_ids:
        one = text if not library else io.StringIO()
        sites._joint_to(one, tables[mid].reshape(-1, len(sites.SEQ_ORDER), len(pack.STRUCT_LETTERS)), mi)
        if library:
            sites.tagged(text, mid, one)
    return text.getvalue()


def main(argv=None, engine=None):
    from . import sites
    args = getoptions(argv)
    if args.iterations < 1:
        fasta.eprint("--iterations: must be at least 1, not %d" % args.iterations)
        return 1
    checked = occupancy_pair.check_inputs(args)
    if checked is None:
        return 1
    with occupancy.Device(engine, args.device, (IOError, expect.ExpectError, sites.InputError)) as dev:
        engine = dev.engine
        recs, srecs, seq_odds, struct_odds, bg_seq, bg_struct = occupancy_pair.sources(args, engine)

        def form_of(odds, pairs):
            """one pass -> per pair (E_seq [m][4], E_struct [m][7][, E_joint [4 m][7], row k * 4 + a]), in code order (pack.RNA_LETTERS,
            pack.STRUCT_LETTERS)"""
            def host(stream, tables, mode):
                if args.joint:
                    eq, es, ej, o, w = engine.expect_pair_joint(stream, tables[0], tables[1], mode)
                    ej = np.asarray(ej)
                    return [eq, es, ej.reshape(ej.shape[:2] + (-1, ej.shape[-1]))], o, w
                eq, es, o, w = engine.expect_pair(stream, tables[0], tables[1], mode)
                return [eq, es], o, w

            def merged(stream, tables, mode, accs):
                got = (engine.expect_pair_joint_merged if args.joint else engine.expect_pair_merged)(stream, tables[0], tables[1], mode, *accs)
                return list(got[:-2]), got[-2], got[-1]
            return expect.Form([sites.pair_id(a, b) for a, b in pairs], occupancy._by_width([odds[0][a].length for a, _ in pairs]), range(len(pairs)),
                               lambda: occupancy_pair.batches(recs, srecs, args.batch_records),
                               lambda m, ks, cols: occupancy_pair.pair_tables(odds[0], odds[1], pairs, ks), host, merged,
                               "expect_pair_joint_merged" if args.joint else "expect_pair_merged",
                               [expect.Matrix(4), expect.Matrix(7)] + ([expect.Matrix(7, rows=4)] if args.joint else []), NOT_FINITE)

        def more(matrices, motif_ids):
            return [(".expected.joint.txt", joint_text(dict((mid, matrices[mid][2]) for mid in motif_ids), motif_ids, args.all_motifs))]

        expect.iterate(args, engine, [expect.Side(".expected.seq.txt", 0, pack.RNA_LETTERS, bg_seq),
                                      expect.Side(".expected.struct.txt", 1, list(pack.STRUCT_LETTERS), bg_struct)],
                       [seq_odds, struct_odds], checked[0], form_of, "motif pairs", more if args.joint else None)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
