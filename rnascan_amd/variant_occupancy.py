"""Threshold-free mutagenesis: how much of a record's occupancy does every single-nucleotide change add or remove.

    python -m rnascan_amd.variant_occupancy -p seq.pfm [-C c] [-u | -b bg] [--all-motifs] [--min-change F] [--effects-only]
                                            [--batch-records n] [--device d] (--variants FILE | --saturate) seqs.fa > table.tsv

``variants`` says which changes create or destroy a site at a threshold ``-m``, through the best window alone; this command
asks the threshold-free family's question: many weak sites count beside one strong one, so what does a letter change do to
their SUM?  The tables are ``occupancy``'s ratio tables.  For a position of a record and a letter a, ``Local.Alt`` is the sum
of the likelihood ratios of the at most m windows over the position if it held a, ``Local.Ref`` the same for the letter it
holds -- ``footprint --weight ratio``'s cover there, bit for bit.  Every other window of the record is
untouched by the change, so the record's occupancy moves by ``Delta = Local.Alt - Local.Ref``.  A change is a ``gain`` when
``Delta > F * Occupancy`` and a ``loss`` when ``Delta < -F * Occupancy`` (both strict); ``--min-change F`` defaults to 0.5: the
change adds or removes more than half of the record's occupancy.

``--variants FILE``: the file of ``variants`` (tab-separated ``Seq_ID  Pos  Ref  Alt``, parsed and checked by its code).  Only
the records the file names are packed; one row per variant (file order) x motif (file order); ``--effects-only`` drops the
``none`` rows.  ``--saturate``: every position x the three other letters; only the ``gain`` and ``loss`` rows, ordered by
record, Pos, Alt in ACGU order, then motif; the decision is taken on the device and only the events come home.

Columns: Motif_ID Seq_ID Pos Ref Alt Occupancy Local.Ref Local.Alt Delta Occupancy.Alt Log2.Fold Effect -- doubles as ``repr``
prints them.  ``Occupancy.Alt = max(fsum([Occupancy, Local.Alt, -Local.Ref]), 0.0)``: the exact combination rounded once, NOT
the summation tree of the mutated record (DESIGN.md 5m bounds the difference); ``Log2.Fold = round(log2(Occupancy.Alt /
Occupancy), 3)``, ``-inf`` for 0.  A record whose occupancy is 0 keeps its rows (any positive Delta is a gain); an infinite or
NaN occupancy is an error that names the motif and the record, and nothing is written.  The bytes do not depend on
``--batch-records``.

Not supported: structure letters, pairs and averaged-structure profiles (the structure side does not follow a letter change
without refolding), insertions and deletions, ``--gpus``.
"""
import argparse
import math
import sys

import numpy as np

from . import fasta, occupancy, pack, variants

COLUMNS = ["Motif_ID", "Seq_ID", "Pos", "Ref", "Alt", "Occupancy", "Local.Ref", "Local.Alt", "Delta", "Occupancy.Alt", "Log2.Fold", "Effect"]
NOT_FINITE = "Motif %s, record %s: the occupancy is infinite or not a number (a ratio of the motif is; check the background and the pseudocount)"


class VariantOccupancyError(ValueError):
    """what the pass found: said on stderr, exit 1, nothing written"""


def classify(ref, alt, occ, frac):
    """-> (Delta: the device's rounded subtraction, again; gain; loss) with lim = frac * occ one rounded product, both compares strict"""
    with np.errstate(all="ignore"):
        delta = np.asarray(alt, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
        lim = np.float64(frac) * np.asarray(occ, dtype=np.float64)
        return delta, delta > lim, delta < -lim


def fold_text(occ, occ_alt):
    """the Log2.Fold column of one row"""
    if occ_alt != occ_alt:
        return "nan"
    if occ == 0.0:
        return "nan" if occ_alt == 0.0 else "inf"
    if occ_alt == 0.0:
        return "-inf"
    return repr(round(math.log2(occ_alt / occ), 3))


def format_row(mid, sid, pos1, ref_code, alt_code, occ, ref, alt, frac):
    """-> (the line, its effect)"""
    occ, ref, alt = float(occ), float(ref), float(alt)
    delta, gain, loss = classify(ref, alt, occ, frac)
    effect = "gain" if gain else "loss" if loss else "none"
    occ_alt = max(math.fsum([occ, alt, -ref]), 0.0) if alt == alt and ref == ref else float("nan")
    line = "%s\t%s\t%d\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n" % (mid, sid, pos1, pack.RNA_LETTERS[ref_code], pack.RNA_LETTERS[alt_code], repr(occ),
                                                           repr(ref), repr(alt), repr(float(delta)), repr(occ_alt), fold_text(occ, occ_alt), effect)
    return line, effect


def _check_finite(occ, motif_ids, ids):
    bad = np.argwhere(~np.isfinite(occ))
    if bad.size:
        raise VariantOccupancyError(NOT_FINITE % (motif_ids[int(bad[0][1])], ids[int(bad[0][0])]))


def saturate_lines(engine, motif_ids, groups, tables, batches, frac):
    """--saturate: the lines of the gain / loss events, batch by batch, in (record, Pos, Alt, motif) order"""
    lines = []
    for ids, stream, _ in batches:
        n_pos = int(np.asarray(stream.codes).size)
        occ = np.zeros((len(ids), len(motif_ids)), dtype=np.float64)
        keys, mos, alts, refs = [], [], [], []
        for m, ks in groups.items():
            key, alt, ref, o, _ = engine.mutocc_events(stream, tables[m], frac)
            occ[:, ks] = np.asarray(o)
            key = np.asarray(key, dtype=np.int64)
            keys.append((key // 4) % max(n_pos, 1) * 4 + (key & 3))    # 4 * position + alt letter
            mos.append(np.asarray(ks, dtype=np.int64)[(key // 4) // max(n_pos, 1)])
            alts.append(np.asarray(alt))
            refs.append(np.asarray(ref))
        _check_finite(occ, motif_ids, ids)
        key, mo, alt, ref = np.concatenate(keys), np.concatenate(mos), np.concatenate(alts), np.concatenate(refs)
        order = np.lexsort((mo, key))
        key, mo, alt, ref = key[order], mo[order], alt[order], ref[order]
        pos = key >> 2
        rec, start = stream.locate(pos)
        codes = np.asarray(stream.codes)
        for i in range(key.size):
            r, k = int(rec[i]), int(mo[i])
            lines.append(format_row(motif_ids[k], ids[r], int(start[i]) + 1, int(codes[pos[i]]) & 7, int(key[i]) & 3, occ[r, k], ref[i], alt[i], frac)[0])
    return lines


def list_lines(engine, recs, motif_ids, groups, tables, path, vlist, frac, batch_records, effects_only):
    """--variants: the lines in (variant, motif) order; only the records the file names are packed, batch by batch of them;
    every file error is raised before a line is kept"""
    from . import scanner
    ids, lengths = list(recs.ids), np.asarray(recs.lengths, dtype=np.int64)
    rec, start = variants.resolve(path, vlist, ids, lengths)
    ref_code = np.asarray([v[3] for v in vlist], dtype=np.uint8)
    alt_code = np.asarray([v[4] for v in vlist], dtype=np.uint8)
    n_var, n_mo = len(vlist), len(motif_ids)
    occ = np.zeros((n_var, n_mo), dtype=np.float64)
    ref = np.zeros((n_var, n_mo), dtype=np.float64)
    alt = np.zeros((n_var, n_mo), dtype=np.float64)
    named = np.unique(rec)
    for a in range(0, named.size, batch_records):
        mine_recs = named[a:a + batch_records]
        batch = scanner._RnaBatch([recs[int(r)] for r in mine_recs])
        stream = pack.Stream(batch.codes, None, batch.offsets, batch.lengths)
        mine = np.flatnonzero(np.isin(rec, mine_recs))
        local_rec = np.searchsorted(mine_recs, rec[mine])
        pos = batch.offsets[local_rec] + start[mine]
        held = batch.codes[pos] & 7
        bad = np.flatnonzero(held != ref_code[mine])
        if bad.size:
            i = int(mine[bad[0]])
            c = int(held[bad[0]])
            raise variants.VariantsError(path, vlist[i][0], "Ref %s is not the letter of record %s at Pos %d (%s)" %
                                         (pack.RNA_LETTERS[ref_code[i]], vlist[i][1], vlist[i][2] + 1, pack.RNA_LETTERS[c] if c < 4 else "not a nucleotide"))
        for m, ks in groups.items():
            local, o, _ = engine.mutocc(stream, tables[m])
            _check_finite(np.asarray(o), [motif_ids[k] for k in ks], [ids[int(r)] for r in mine_recs])
            for x, k in enumerate(ks):
                occ[mine, k] = np.asarray(o)[local_rec, x]
                ref[mine, k] = local[x, pos, ref_code[mine]]
                alt[mine, k] = local[x, pos, alt_code[mine]]
    lines = []
    for i in range(n_var):
        for k, mid in enumerate(motif_ids):
            line, effect = format_row(mid, vlist[i][1], int(start[i]) + 1, int(ref_code[i]), int(alt_code[i]), occ[i, k], ref[i, k], alt[i, k], frac)
            if not effects_only or effect != "none":
                lines.append(line)
    return lines


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.variant_occupancy",
                                     description=("Threshold-free mutagenesis: the single-nucleotide changes that add or remove more than a "
                                                  "share of a record's occupancy under a sequence motif."))
    parser.add_argument("inputs", metavar="seqs.fa", nargs="+", help="the sequence FASTA")
    occupancy.add_options(parser, ["-p", "-C", "-u", "-b", "--all-motifs"], every="motif of a multi-PFM file")
    parser.add_argument("--min-change", type=float, default=0.5, dest="min_change", metavar="F",
                        help="a change is a gain or a loss when it moves the occupancy by more than F times the record's occupancy [%(default)s]")
    parser.add_argument("--effects-only", action="store_true", default=False, dest="effects_only", help="with --variants: only the gain and loss rows [off]")
    occupancy.add_options(parser, ["--batch-records", "--device"], result="output does")
    mode = parser.add_mutually_exclusive_group(required=True)
    mode.add_argument("--variants", dest="variants", metavar="FILE", help="tab-separated Seq_ID, Pos (1-based), Ref, Alt")
    mode.add_argument("--saturate", action="store_true", default=False, help="every position x the three other letters; gain and loss rows only")
    args = parser.parse_intermixed_args(argv)
    args.pfm_struct = args.bg_struct = None
    args.struct_format = "auto"
    occupancy.check_options(parser, args)
    if not args.pfm_seq:
        parser.error("-p (sequence PFM) is required")
    if not args.min_change >= 0:
        parser.error("--min-change: must be a number that is not negative")
    args.fasta = args.inputs[0]
    return args


def main(argv=None, engine=None, out=None):
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    if len(args.inputs) != 1:
        fasta.eprint("one input: the sequence FASTA (the structure side does not follow a letter change without refolding)")
        return 1
    if occupancy._is_profiles(args.fasta):
        fasta.eprint("%s is an averaged-structure directory or packed store: a letter change does not carry over to the structure "
                     "without refolding, give the sequence FASTA" % args.fasta)
        return 1
    with occupancy.Device(engine, args.device, (IOError, variants.VariantsError, VariantOccupancyError)) as dev:
        vlist = variants.parse_variants(args.variants) if args.variants else None
        got = occupancy.single_fasta(args, dev)
        if got is None:
            return 1
        motif_ids, letters, code_letters, _, odds, recs = got
        engine = dev.engine
        groups = occupancy._by_width([odds[mid].length for mid in motif_ids])
        tables = dict((m, np.stack([odds[motif_ids[k]].ratio_table(code_letters) for k in ks])) for m, ks in groups.items())
        frac = float(args.min_change)
        if vlist is not None:
            lines = list_lines(engine, recs, motif_ids, groups, tables, args.variants, vlist, frac, args.batch_records, args.effects_only)
        else:
            lines = saturate_lines(engine, motif_ids, groups, tables, occupancy.letter_batches(recs, letters, args.batch_records), frac)
        # every line is made before the first is written: a record that fails leaves nothing behind
        out.write("\t".join(COLUMNS) + "\n")
        out.write("".join(lines))
        out.flush()
        fasta.eprint("Wrote %d rows" % len(lines))
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
