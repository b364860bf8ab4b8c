"""Occupancy: how much of each motif does each record carry -- a records x motifs table, no threshold.

    python -m rnascan_amd.occupancy (-p seq.pfm | -q struct.pfm) [-C c] [-u | -b bg | -B bg] [--all-motifs]
                                    [--struct-format auto|letters|dotbracket] [--device N] in.fa > table.tsv

The occupancy (summed affinity) of a record under a motif is the sum over its windows of the window's likelihood ratio
prod_k p_k(x) / b(x) = 2 ** score, taken from the PFM's own odds ratios (``pssm.odds``: what ``rnascan`` takes the log of)
without any ``exp`` or ``log``: a sequential fp64 product per window and a fixed summation tree per record,
the same bits whatever the batch size.  A window with a foreign letter has no term and is not counted in ``Windows``.

``-p`` takes a sequence FASTA, ``-q`` a structure-letter FASTA; dot-bracket structures are annotated on the GPU first,
exactly as ``rnascan -q`` does (``--struct-format``).  The background is computed from the input unless ``-u`` or a
background file says otherwise, as ``rnascan`` does.

One row per record x motif, in record order and then the file's motif order (the first motif of a multi-PFM file; every
motif with ``--all-motifs``).  Columns: Motif_ID Seq_ID Windows Occupancy Log2.Occupancy -- ``Occupancy`` as ``repr`` prints
the double (the shortest string that reads back to the same bits), ``Log2.Occupancy = round(log2(occ), 3)``, ``-inf`` for 0.
A record shorter than the motif gets its row with ``Windows`` 0 and ``Occupancy`` 0.0.
"""
import argparse
import math
import os
import sys

import numpy as np

from . import fasta, pack

COLUMNS = ["Motif_ID", "Seq_ID", "Windows", "Occupancy", "Log2.Occupancy"]
BATCH_RECORDS = 4096                                 # records per packed batch (and per device call); the output does not depend on it


def log2_text(x):
    """the Log2.Occupancy column of one value"""
    x = float(x)
    if x != x:
        return "nan"
    if x == 0.0:
        return "-inf"
    return repr(round(math.log2(x), 3))


def format_rows(motif_ids, seq_ids, windows, occ):
    """the table's lines (no header) for occ float64 [n_rec][n_motifs] and windows int64 [n_rec][n_motifs]"""
    lines = []
    for r, sid in enumerate(seq_ids):
        for k, mid in enumerate(motif_ids):
            x = float(occ[r, k])
            lines.append("%s\t%s\t%d\t%s\t%s\n" % (mid, sid, int(windows[r, k]), repr(x), log2_text(x)))
    return lines


def run(engine, out, recs, odds, motif_ids, letters, code_letters, batch_records=BATCH_RECORDS):
    """rows in (record, motif) order, batch by batch of records; one device call per batch and width"""
    from . import scanner
    n_letters = len(code_letters)
    groups = {}
    for k, mid in enumerate(motif_ids):
        groups.setdefault(odds[mid].length, []).append(k)
    tables = dict((m, np.stack([odds[motif_ids[k]].ratio_table(code_letters) for k in ks])) for m, ks in groups.items())
    total = 0
    for a in range(0, len(recs), batch_records):
        b = min(len(recs), a + batch_records)
        batch = scanner._RnaBatch(recs[a:b], None if letters == fasta.RNA else letters)
        if len(batch) == 0:
            continue
        stream = pack.Stream(batch.codes, None, batch.offsets, batch.lengths)
        occ = np.zeros((len(batch), len(motif_ids)), dtype=np.float64)
        win = np.zeros((len(batch), len(motif_ids)), dtype=np.int64)
        for m, ks in groups.items():
            o, w = engine.occupancy(stream, tables[m], n_letters)
            occ[:, ks] = o
            win[:, ks] = w[:, None]
        out.write("".join(format_rows(motif_ids, list(batch.ids), win, occ)))
        total += len(batch) * len(motif_ids)
    return total


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.occupancy",
                                     description=("Occupancy: the summed likelihood ratio of every record under every motif, "
                                                  "a threshold-free records x motifs table."))
    parser.add_argument("fasta", metavar="in.fa", help="the sequence FASTA (-p) or structure FASTA (-q)")
    parser.add_argument("-p", "--pfm_seq", dest="pfm_seq", type=str, default=None, help="Sequence PFM")
    parser.add_argument("-q", "--pfm_struct", dest="pfm_struct", type=str, default=None, help="Structure PFM")
    parser.add_argument("-C", "--pseudocount", type=float, dest="pseudocount", default=0, help="Pseudocount for normalizing PFM. [%(default)s]")
    parser.add_argument("-u", "--uniformbg", action="store_true", default=False, dest="uniform_background",
                        help="Use uniform background for the odds ratios [%(default)s]")
    parser.add_argument("-b", "--bg_seq", default=None, dest="bg_seq", help="File of pre-computed background probabilities for sequences")
    parser.add_argument("-B", "--bg_struct", default=None, dest="bg_struct", help="File of pre-computed background probabilities for structures")
    parser.add_argument("--all-motifs", action="store_true", default=False, dest="all_motifs", help="every motif of a multi-PFM file, one call per width [off]")
    parser.add_argument("--struct-format", choices=["auto", "letters", "dotbracket"], default="auto", dest="struct_format",
                        help="-q: what the structure FASTA holds; dot-bracket strings are annotated on the GPU first [%(default)s]")
    parser.add_argument("--batch-records", type=int, default=BATCH_RECORDS, dest="batch_records",
                        help="records per device call; the table does not depend on it [%(default)s]")
    parser.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")
    args = parser.parse_args(argv)
    if args.uniform_background and (args.bg_seq or args.bg_struct):
        parser.error("You cannot set uniform and custom background options at the same time\n")
    if args.batch_records < 1:
        parser.error("--batch-records: must be positive")
    return args


def main(argv=None, engine=None, out=None):
    from . import cli, pssm, scanner
    from ._lib import MAX_M
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    if args.pfm_seq and args.pfm_struct:
        fasta.eprint("-p and -q cannot be given together: the occupancy of two-FASTA pairs is not supported, run one at a time")
        return 1
    if not args.pfm_seq and not args.pfm_struct:
        fasta.eprint("one of -p (sequence PFM) or -q (structure PFM) is required")
        return 1
    seq = bool(args.pfm_seq)
    option, pfm_file = ("-p", args.pfm_seq) if seq else ("-q", args.pfm_struct)
    letters, code_letters = (fasta.RNA, pack.RNA_LETTERS) if seq else (fasta.STRUCT, pack.STRUCT_LETTERS)
    own = engine is None
    try:
        try:
            shapes = pssm.load_odds(pfm_file, args.pseudocount, letters, None)      # widths only: before any device work
        except KeyError:
            fasta.eprint("Failed to load motif %s (%s): check that the PFM has the letters %s" % (pfm_file, option, letters))
            return 1
        if not shapes:
            fasta.eprint("No motif could be read from %s (%s)" % (pfm_file, option))
            return 1
        motif_ids = list(shapes.keys()) if args.all_motifs else [next(iter(shapes))]
        for mid in motif_ids:
            if shapes[mid].length > MAX_M:
                fasta.eprint("%s: motif %s of %s is %d positions wide, more than %d (PFMSCAN_MAX_M)" %
                             (option, mid, pfm_file, shapes[mid].length, MAX_M))
                return 1
        if engine is None:
            engine = scanner.HipEngine(args.device)
        source = args.fasta
        if not seq:
            # a dot-bracket structure FASTA is annotated first and replaced by its letters (cli.struct_input)
            ns = argparse.Namespace(fastafiles=[args.fasta], struct_format=args.struct_format, testseq=None)
            cli.struct_input(ns, "SS", None, lambda: engine)
            source = ns.fastafiles[0]
        bg = fasta.load_background(args.bg_seq if seq else args.bg_struct, args.uniform_background, source, letters, True)
        odds = pssm.load_odds(pfm_file, args.pseudocount, letters, bg)
        recs = fasta.open_lazy(source)
        out.write("\t".join(COLUMNS) + "\n")
        n = run(engine, out, recs, odds, motif_ids, letters, code_letters, args.batch_records)
        out.flush()
        fasta.eprint("Wrote %d rows" % n)
        return 0
    except IOError as e:
        fasta.eprint(str(e))
        return 1
    finally:
        if own and engine is not None:
            engine.close()


if __name__ == "__main__":
    sys.exit(main())
