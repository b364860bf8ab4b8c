"""Occupancy of sequence + structure FASTA pairs: how much of each sequence-and-structure motif does each record carry.

    python -m rnascan_amd.occupancy_pair -p seq.pfm -q struct.pfm [-C c] [-u | -b bg -B bg] [--all-motifs]
                                         [--struct-format auto|letters|dotbracket] [--batch-records n] [--device d]
                                         seqs.fa structs.fa > table.tsv

The fourth input mode of ``rnascan``: the structure of a record is a string of structure letters, one per nucleotide (one
fold per transcript, or a dot-bracket file, which is annotated on the GPU first as ``rnascan -q`` does).  The ratio of a
window is the product of its sequence ratio and its structure ratio -- the ratio behind ``LogOdds.SeqStruct`` -- and the
occupancy of a record is the sum of these products over its windows.  A sum of products is not a product of sums: the
table cannot be made from ``occupancy -p`` and ``occupancy -q``.  The arithmetic is ``occupancy``'s, the joint
chain that of DESIGN.md 5j: the sequence letters, then the structure letters, every product rounded, a fixed summation tree
per record, the same bits whatever the batch size.  A window with a foreign letter in either file has no term and is not
counted in ``Windows``.

The two files hold the same ids in the same order with equal lengths (``sites`` pairs them the same way); the motifs of two
libraries are paired as ``rnascan`` pairs them and named as the site profiles name a pair; the backgrounds are resolved
per side exactly as ``occupancy -p`` and ``occupancy -q`` resolve them.  Columns and formatting are ``occupancy``'s:
Motif_ID Seq_ID Windows Occupancy Log2.Occupancy.
"""
import argparse
import sys

import numpy as np

from . import fasta, occupancy, pack

COLUMNS = occupancy.COLUMNS
BATCH_RECORDS = occupancy.BATCH_RECORDS


def add_options(parser, options=occupancy.OPTIONS):
    """the options ``occupancy_pair`` and ``expect_pair`` share"""
    parser.add_argument("inputs", metavar="input", nargs="+", help="the sequence FASTA and the structure FASTA (letters or dot-bracket)")
    occupancy.add_options(parser, ["-p", "-q", "-C", "-u", "-b", "-B", "--all-motifs", "--struct-format", "--batch-records", "--device"], options,
                          every="pair of multi-PFM files", q="", result="output does")


def check_inputs(args):
    """everything that can be refused before a device is opened -> (pairs, seq_shapes, struct_shapes) or None (said on
    stderr): both PFMs and two FASTA files given, the libraries paired (pairs of unequal width and widths above
    PFMSCAN_MAX_M are errors that name the motif), the two files matched record by record"""
    from . import sites
    if not args.pfm_seq or not args.pfm_struct:
        fasta.eprint("both -p (sequence PFM) and -q (structure PFM) are required: one of them alone is `python -m rnascan_amd.%s`" % args.single)
        return None
    if len(args.inputs) != 2:
        fasta.eprint("two inputs are required: the sequence FASTA and the structure FASTA (seqs.fa structs.fa)")
        return None
    for path in args.inputs:
        if occupancy._is_profiles(path):
            fasta.eprint("%s is an averaged-structure directory or packed store: that input mode is `python -m rnascan_amd.%s`" % (path, args.profiles))
            return None
    motifs = occupancy.profile_motifs(args)
    if motifs is None:
        return None
    try:
        sites.paired_fastas(args.inputs[0], args.inputs[1])
    except (IOError, sites.InputError) as e:
        fasta.eprint(str(e))
        return None
    pairs, st_shapes, seq_shapes = motifs
    return pairs, seq_shapes, st_shapes


def sources(args, engine):
    """once a device is open: the structure FASTA annotated if it holds dot-bracket strings (cli.struct_input), the two files
    matched again, the backgrounds resolved per side as ``occupancy -p`` / ``-q`` resolve them ->
    (recs, srecs, seq_odds, struct_odds, bg_seq, bg_struct)"""
    from . import cli, pssm, sites
    ns = argparse.Namespace(fastafiles=list(args.inputs), struct_format=args.struct_format, testseq=None)
    cli.struct_input(ns, "RNASS", None, lambda: engine)
    seq_file, struct_file = ns.fastafiles
    recs, srecs = sites.paired_fastas(seq_file, struct_file)
    bg_seq = fasta.load_background(args.bg_seq, args.uniform_background, seq_file, fasta.RNA, True)
    bg_struct = fasta.load_background(args.bg_struct, args.uniform_background, struct_file, fasta.STRUCT, True)
    seq_odds = pssm.load_odds(args.pfm_seq, args.pseudocount, fasta.RNA, bg_seq)
    struct_odds = pssm.load_odds(args.pfm_struct, args.pseudocount, fasta.STRUCT, bg_struct)
    return recs, srecs, seq_odds, struct_odds, bg_seq, bg_struct


def batches(recs, srecs, batch_records):
    """(ids, pack.Stream with codes and codes2, None) of every batch of records that holds one: the third batch source beside
    ``occupancy.letter_batches`` and ``occupancy.profile_batches``"""
    from . import scanner, sites
    for a in range(0, len(recs), batch_records):
        b = min(len(recs), a + batch_records)
        sb, tb = scanner._RnaBatch(recs[a:b]), scanner._RnaBatch(srecs[a:b], fasta.STRUCT)
        if len(sb) == 0:
            continue
        if not np.array_equal(sb.lengths, tb.lengths):
            r = int(np.flatnonzero(sb.lengths != tb.lengths)[0])
            raise sites.InputError("record %s is %d letters long but its structure string has %d" %
                                   (sb.ids[r], int(sb.lengths[r]), int(tb.lengths[r])))
        yield list(sb.ids), pack.Stream(sb.codes, None, sb.offsets, sb.lengths, codes2=tb.codes), None


def pair_tables(seq_odds, struct_odds, pairs, ks):
    """the two table stacks [len(ks)][m][8] of the pairs ks (one width)"""
    return (np.stack([seq_odds[pairs[k][0]].ratio_table(pack.RNA_LETTERS) for k in ks]),
            np.stack([struct_odds[pairs[k][1]].ratio_table(pack.STRUCT_LETTERS) for k in ks]))


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.occupancy_pair",
                                     description=("Occupancy of sequence + structure FASTA pairs: the summed joint likelihood ratio of "
                                                  "every record under every motif pair, a threshold-free records x pairs table."))
    add_options(parser)
    args = parser.parse_intermixed_args(argv)
    occupancy.check_options(parser, args)
    args.single, args.profiles = "occupancy", "occupancy"
    return args


def main(argv=None, engine=None, out=None):
    from . import sites
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    checked = check_inputs(args)
    if checked is None:
        return 1
    pairs = checked[0]
    with occupancy.Device(engine, args.device, (IOError, sites.InputError)) as dev:
        engine = dev.engine
        recs, srecs, seq_odds, struct_odds, _, _ = sources(args, engine)
        groups = occupancy._by_width([seq_odds[a].length for a, _ in pairs])
        tables = dict((m, pair_tables(seq_odds, struct_odds, pairs, ks)) for m, ks in groups.items())
        occupancy.write_table(out, [sites.pair_id(a, b) for a, b in pairs], groups, batches(recs, srecs, args.batch_records),
                              lambda stream, m, ks, cols: engine.occupancy_pair(stream, *tables[m]))
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
