"""Footprint: where in each record does the motif bind -- per-position posterior site coverage, no threshold on the score.

    python -m rnascan_amd.footprint (-p seq.pfm | -q struct.pfm | -p seq.pfm -q struct.pfm) [-C c] [-u | -b bg | -B bg]
                                    [--weight posterior|ratio] [--min-cover T] [--positions] [--all-motifs]
                                    [--struct-format auto|letters|dotbracket] [--batch-records n] [--device d]
                                    in.fa [structs.fa] > regions.tsv

Every window of a record is weighted as ``expect`` weights it: by its likelihood ratio under the motif (``--weight ratio``) or
by that ratio over the record's occupancy (``--weight posterior``, the default: one site per record in expectation).  The
cover of a position is the sum of the weights of the at most m windows that lie over it, added in ascending order of their
starts; with posterior weights it is the probability that the position lies under the site.  The weights and
the covers are made on the GPU with the family's arithmetic -- a sequential fp64 product per window, one rounded division
per record, m rounded additions per position -- and only the positions whose cover is greater than ``--min-cover`` come home,
so the bytes written do not depend on ``--batch-records``.

``-p`` takes a sequence FASTA, ``-q`` a structure-letter FASTA (dot-bracket structures are annotated on the GPU first, as
``occupancy -q`` does), ``-p`` with ``-q`` the two FASTA files of ``occupancy_pair``, checked as it checks them.

One row per region, a maximal run of consecutive positions of a record with cover > T, in record order, then the file's motif
order, then position.  Columns: Motif_ID Seq_ID Start End Peak.Pos Peak.Cover Mass -- ``Start`` and ``End`` 1-based inclusive
as ``rnascan``'s, ``Peak.Pos`` the lowest position of greatest cover, ``Mass`` the ``math.fsum`` of the weights of the windows
that lie wholly inside the region (those that start in [Start, End - m + 1]; 0.0 when there is none): with posterior weights
the probability that the site lies inside the region.  ``--positions``: one row per position instead, Motif_ID Seq_ID Pos
Start.Weight Cover.  Doubles are printed with ``repr``.  ``--min-cover`` is 0.5 with posterior weights and has to be given
with ``--weight ratio``, which has no natural scale.  A record whose occupancy is 0 has no row (how many is said on stderr); an
infinite or NaN occupancy is an error that names the motif and the record, and nothing is written.

Not supported: averaged-structure profiles (they are ``python -m rnascan_amd.footprint_profile``), ``--gpus``, bedGraph or bigWig output, merging
regions on the device, more or fewer than one site per record (ZOOPS).
"""
import argparse
import math
import sys

import numpy as np

from . import expect, fasta, occupancy, occupancy_pair

COLUMNS = ["Motif_ID", "Seq_ID", "Start", "End", "Peak.Pos", "Peak.Cover", "Mass"]
POSITION_COLUMNS = ["Motif_ID", "Seq_ID", "Pos", "Start.Weight", "Cover"]
MODES = expect.MODES
NOT_FINITE = "Motif %s, record %s: the occupancy is infinite or not a number (a ratio of the motif is; check the background and the pseudocount)"


class FootprintError(ValueError):
    """what the pass found: said on stderr, exit 1, nothing written"""


def regions(pos, cover, start, m):
    """the regions of one record under one motif from its events: pos int (0-based, ascending), their cover and start weight ->
    [(first, last, peak, peak cover, mass)], 0-based inclusive"""
    out = []
    n = len(pos)
    a = 0
    while a < n:
        b = a
        while b + 1 < n and pos[b + 1] == pos[b] + 1:
            b += 1
        first, last = int(pos[a]), int(pos[b])
        peak = a
        for i in range(a + 1, b + 1):
            if cover[i] > cover[peak]:                             # strict: the lowest position of greatest cover
                peak = i
        inside = [float(start[i]) for i in range(a, b + 1) if pos[i] <= last - m + 1]
        out.append((first, last, int(pos[peak]), float(cover[peak]), math.fsum(inside) if inside else 0.0))
        a = b + 1
    return out


def format_rows(mid, sid, pos, cover, start, m, positions):
    """the lines of one record under one motif"""
    if positions:
        return ["%s\t%s\t%d\t%s\t%s\n" % (mid, sid, int(p) + 1, repr(float(w)), repr(float(c))) for p, c, w in zip(pos, cover, start)]
    return ["%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (mid, sid, first + 1, last + 1, peak + 1, repr(c), repr(mass))
            for first, last, peak, c, mass in regions(pos, cover, start, m)]


def batch_rows(motif_ids, groups, ids, stream, call, positions, cols=None):
    """the lines of one batch in (record, motif, position) order, and how many (record, motif) have occupancy 0.
    ``call(stream, m, ks)`` -> (key, cover, start, occ [n_rec][len(ks)], windows); a batch of averaged-structure profiles
    comes with its stored column order and is ``call(stream, m, ks, cols)``"""
    n_pos = int(np.asarray(stream.codes).size) if stream.codes is not None else int(np.asarray(stream.profile).shape[0])
    offsets = np.asarray(stream.offsets, dtype=np.int64)
    got = {}                                                       # (record, motif) -> (positions in the record, cover, start, width)
    occ = np.zeros((len(ids), len(motif_ids)), dtype=np.float64)
    for m, ks in groups.items():
        key, cover, start, o, _ = call(stream, m, ks) if cols is None else call(stream, m, ks, cols)
        occ[:, ks] = np.asarray(o)
        key = np.asarray(key, dtype=np.int64)
        j, p = key // max(n_pos, 1), key % max(n_pos, 1)
        r = np.searchsorted(offsets, p, side="right") - 1
        # the keys are sorted: motif, then position, so the events of a (motif, record) are a run
        cut = np.flatnonzero((np.diff(j) != 0) | (np.diff(r) != 0)) + 1 if key.size else np.zeros(0, dtype=np.int64)
        for a, b in zip(np.concatenate([[0], cut]).astype(int), np.concatenate([cut, [key.size]]).astype(int)):
            if b > a:
                got[(int(r[a]), ks[int(j[a])])] = (p[a:b] - offsets[r[a]], cover[a:b], start[a:b], m)
    bad = np.argwhere(~np.isfinite(occ))
    if bad.size:
        raise FootprintError(NOT_FINITE % (motif_ids[int(bad[0][1])], ids[int(bad[0][0])]))
    lines = []
    for r, sid in enumerate(ids):
        for k, mid in enumerate(motif_ids):
            if (r, k) in got and occ[r, k] != 0.0:
                pos, cover, start, m = got[(r, k)]
                lines += format_rows(mid, sid, pos, cover, start, m, positions)
    return lines, int((occ == 0.0).sum())


def write_table(out, motif_ids, groups, batches, call, positions):
    """every line is made before the first is written: a record that fails leaves nothing behind"""
    lines, empty = [], 0
    for ids, stream, cols in batches:
        more, zero = batch_rows(motif_ids, groups, ids, stream, call, positions, cols)
        lines += more
        empty += zero
    out.write("\t".join(POSITION_COLUMNS if positions else COLUMNS) + "\n")
    out.write("".join(lines))
    out.flush()
    if empty:
        fasta.eprint("%d record x motif pairs have occupancy 0 and no row" % empty)
    fasta.eprint("Wrote %d rows" % len(lines))


OPTIONS = dict(expect.OPTIONS)
OPTIONS.update({
    "--min-cover": lambda p, w: p.add_argument("--min-cover", type=float, default=None, dest="min_cover", metavar="T",
                                               help="report the positions whose cover is greater than T [0.5 with --weight posterior; required with --weight ratio]"),
    "--positions": lambda p, w: p.add_argument("--positions", action="store_true", default=False,
                                               help="one row per position with cover > T instead of one per region [off]"),
})


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.footprint",
                                     description=("Footprint: the posterior site coverage of every position, reported as the regions "
                                                  "(or positions) whose cover passes --min-cover.  No threshold on the score."))
    parser.add_argument("inputs", metavar="input", nargs="+",
                        help="the sequence FASTA (-p) or structure FASTA (-q); or both, sequences first (-p with -q)")
    occupancy.add_options(parser, ["-p", "-q", "-C", "-u", "-b", "-B", "--weight", "--min-cover", "--positions", "--all-motifs", "--struct-format",
                                   "--batch-records", "--device"], OPTIONS, every="motif (or pair) of multi-PFM files", q="", result="output does",
                          joint="")
    args = parser.parse_intermixed_args(argv)
    occupancy.check_options(parser, args)
    if args.min_cover is None:
        if args.weight != "posterior":
            parser.error("--min-cover is required with --weight ratio: likelihood ratios have no natural scale")
        args.min_cover = 0.5
    if args.min_cover != args.min_cover:
        parser.error("--min-cover: not a number")
    args.single, args.profiles = "footprint", "occupancy"
    args.fasta = args.inputs[0]
    return args


def main(argv=None, engine=None, out=None):
    from . import sites
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    mode = MODES[args.weight]
    if not args.pfm_seq and not args.pfm_struct:
        fasta.eprint("one of -p (sequence PFM) or -q (structure PFM), or both, is required")
        return 1
    pair = bool(args.pfm_seq) and bool(args.pfm_struct)
    if pair:
        checked = occupancy_pair.check_inputs(args)
        if checked is None:
            return 1
    else:
        if len(args.inputs) != 1:
            fasta.eprint("%s alone takes one input: give -p and -q with the sequence FASTA and the structure FASTA" % ("-p" if args.pfm_seq else "-q"))
            return 1
        if occupancy._is_profiles(args.fasta):
            fasta.eprint("%s is an averaged-structure directory or packed store: footprints take FASTA files of letters "
                         "(averaged-structure profiles are `python -m rnascan_amd.footprint_profile`)" % args.fasta)
            return 1
    with occupancy.Device(engine, args.device, (IOError, sites.InputError, FootprintError)) as dev:
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
        write_table(out, motif_ids, groups, batches,
                    lambda stream, m, ks: engine.footprint_events(stream, tables[m][0], tables[m][1], mode, args.min_cover), args.positions)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
