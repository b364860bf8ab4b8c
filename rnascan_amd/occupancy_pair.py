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
import os
import sys

import numpy as np

from . import fasta, occupancy, pack

COLUMNS = occupancy.COLUMNS
BATCH_RECORDS = occupancy.BATCH_RECORDS


def add_options(parser):
    """the options ``occupancy_pair`` and ``expect_pair`` share"""
    parser.add_argument("inputs", metavar="input", nargs="+", help="the sequence FASTA and the structure FASTA (letters or dot-bracket)")
    parser.add_argument("-p", "--pfm_seq", dest="pfm_seq", type=str, default=None, help="Sequence PFM")
    parser.add_argument("-q", "--pfm_struct", dest="pfm_struct", type=str, default=None, help="Structure PFM")
    parser.add_argument("-C", "--pseudocount", type=float, dest="pseudocount", default=0, help="Pseudocount for normalizing PFM. [%(default)s]")
    parser.add_argument("-u", "--uniformbg", action="store_true", default=False, dest="uniform_background",
                        help="Use uniform background for the odds ratios [%(default)s]")
    parser.add_argument("-b", "--bg_seq", default=None, dest="bg_seq", help="File of pre-computed background probabilities for sequences")
    parser.add_argument("-B", "--bg_struct", default=None, dest="bg_struct", help="File of pre-computed background probabilities for structures")
    parser.add_argument("--all-motifs", action="store_true", default=False, dest="all_motifs", help="every pair of multi-PFM files, one call per width [off]")
    parser.add_argument("--struct-format", choices=["auto", "letters", "dotbracket"], default="auto", dest="struct_format",
                        help="what the structure FASTA holds; dot-bracket strings are annotated on the GPU first [%(default)s]")
    parser.add_argument("--batch-records", type=int, default=BATCH_RECORDS, dest="batch_records",
                        help="records per device call; the output does not depend on it [%(default)s]")
    parser.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")


def check_options(parser, args):
    if args.uniform_background and (args.bg_seq or args.bg_struct):
        parser.error("You cannot set uniform and custom background options at the same time\n")
    if args.batch_records < 1:
        parser.error("--batch-records: must be positive")


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
    """(ids, pack.Stream with codes and codes2) of every batch of records that holds one"""
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
        yield list(sb.ids), pack.Stream(sb.codes, None, sb.offsets, sb.lengths, codes2=tb.codes)


def pair_tables(seq_odds, struct_odds, pairs, ks):
    """the two table stacks [len(ks)][m][8] of the pairs ks (one width)"""
    return (np.stack([seq_odds[pairs[k][0]].ratio_table(pack.RNA_LETTERS) for k in ks]),
            np.stack([struct_odds[pairs[k][1]].ratio_table(pack.STRUCT_LETTERS) for k in ks]))


def run(engine, out, recs, srecs, seq_odds, struct_odds, pairs, batch_records=BATCH_RECORDS):
    """rows in (record, pair) order, batch by batch of records; one device call per batch and width"""
    from . import sites
    motif_ids = [sites.pair_id(a, b) for a, b in pairs]
    groups = occupancy._by_width([seq_odds[a].length for a, _ in pairs])
    tables = dict((m, pair_tables(seq_odds, struct_odds, pairs, ks)) for m, ks in groups.items())
    total = 0
    for ids, stream in batches(recs, srecs, batch_records):
        occ = np.zeros((len(ids), len(pairs)), dtype=np.float64)
        win = np.zeros((len(ids), len(pairs)), dtype=np.int64)
        for m, ks in groups.items():
            o, w = engine.occupancy_pair(stream, tables[m][0], tables[m][1])
            occ[:, ks] = o
            win[:, ks] = np.asarray(w)[:, None]
        out.write("".join(occupancy.format_rows(motif_ids, ids, win, occ)))
        total += len(ids) * len(pairs)
    return total


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.occupancy_pair",
                                     description=("Occupancy of sequence + structure FASTA pairs: the summed joint likelihood ratio of "
                                                  "every record under every motif pair, a threshold-free records x pairs table."))
    add_options(parser)
    args = parser.parse_intermixed_args(argv)
    check_options(parser, args)
    args.single, args.profiles = "occupancy", "occupancy"
    return args


def main(argv=None, engine=None, out=None):
    from . import scanner, sites
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    checked = check_inputs(args)
    if checked is None:
        return 1
    pairs = checked[0]
    own = engine is None
    try:
        if engine is None:
            engine = scanner.HipEngine(args.device)
        recs, srecs, seq_odds, struct_odds, _, _ = sources(args, engine)
        out.write("\t".join(COLUMNS) + "\n")
        n = run(engine, out, recs, srecs, seq_odds, struct_odds, pairs, args.batch_records)
        out.flush()
        fasta.eprint("Wrote %d rows" % n)
        return 0
    except (IOError, sites.InputError) as e:
        fasta.eprint(str(e))
        return 1
    finally:
        if own and engine is not None:
            engine.close()


if __name__ == "__main__":
    sys.exit(main())
