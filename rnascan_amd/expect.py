"""Expected site counts: one EM step (or several) of motif refinement, without a threshold.

    python -m rnascan_amd.expect (-p seq.pfm | -q struct.pfm) [-C c] [-u | -b bg | -B bg] [--weight posterior|ratio]
                                 [--iterations N] [--all-motifs] [--struct-format auto|letters|dotbracket]
                                 [--batch-records n] [--merge auto|device|host] [--device d] -o PREFIX in.fa

Every window of every record is weighted by its likelihood ratio prod_k p_k(x) / b(x) under the motif (``--weight ratio``)
or by that ratio over the record's occupancy, the sum of the ratios of all its windows (``--weight posterior``, the default:
every record carries one site in expectation, the OOPS model's E-step).  The letters under the windows are added up with
these weights: ``E[k][c]`` is the expected number of times letter ``c`` lies under motif column ``k``.  The weights and the
per-record sums are made on the GPU with the occupancy's arithmetic -- a sequential fp64 product per window, one rounded
division per record, a fixed summation tree per record -- and the records are added up exactly, on the device
in long integer accumulators or on the host with ``math.fsum`` (``--merge``, DESIGN.md 5k: the same bytes either way), so
the bytes written do not depend on ``--batch-records`` or on the order of the records.

``PREFIX.expected.txt`` holds ``E`` as a PFM that ``-p`` / ``-q`` of ``rnascan``, ``sites``, ``occupancy`` and this command
read (a multi-PFM library in the file's motif order with ``--all-motifs``; the file's first motif otherwise), every number in
the shortest form that reads back to the same double.  ``PREFIX.summary.txt`` has one line per motif and iteration:
Motif_ID Iteration Records Records.Skipped Windows Log2.Likelihood -- the records with an occupancy > 0, those with
occupancy 0 (no window with a term, or every ratio 0), the windows with a term, and the sum of log2(occupancy) over the
counted records, rounded to 3 places (reporting only).

``--iterations N``: iteration i + 1 takes the E of iteration i as its count matrix, normalised with the same pseudocount
against the same background -- what reading iteration i's file would give, so ``--iterations 2`` writes the bytes of a run
on the output of a run.

``-p`` takes a sequence FASTA, ``-q`` a structure-letter FASTA; dot-bracket structures are annotated on the GPU first, as
``occupancy -q`` does.  Averaged-structure profiles are ``python -m rnascan_amd.expect_profile``, two-FASTA pairs
``python -m rnascan_amd.expect_pair``.  Not supported: ``--gpus``, priors other than one site per record, convergence criteria, a
change of the motif's width.
"""
import argparse
import io
import math
import os
import sys
from collections import OrderedDict

import numpy as np

from . import fasta, pack

COLUMNS = ["Motif_ID", "Iteration", "Records", "Records.Skipped", "Windows", "Log2.Likelihood"]
BATCH_RECORDS = 4096                                 # records per packed batch (and per device call); the output does not depend on it
MODES = {"ratio": 0, "posterior": 1}                 # _lib.EXPECT_RATIO, _lib.EXPECT_POSTERIOR


class ExpectError(ValueError):
    """what the pass found: said on stderr, exit 1, nothing written"""


def fsum_records(parts):
    """parts: arrays [n_rec_i][m][n] -> their exact sum over all records, float64 [m][n] (math.fsum per cell)"""
    X = np.concatenate(parts, axis=0)
    out = np.zeros(X.shape[1:], dtype=np.float64)
    for k in range(X.shape[1]):
        for c in range(X.shape[2]):
            out[k, c] = math.fsum(X[:, k, c].tolist())
    return out


MERGES = ("auto", "device", "host")                  # --merge: where the records are added up
NOT_FINITE = ("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
              "(a ratio of the motif is; check the background and the pseudocount)")


class NegativeCell(ExpectError):
    """the device route met a cell < 0, which the long accumulator cannot hold"""


def add_merge_option(parser):
    parser.add_argument("--merge", choices=MERGES, default="auto",
                        help="where the records are added up: exactly on the device (long accumulators), or on the host with "
                             "math.fsum; the files do not depend on it [%(default)s: device where the engine offers it]")


def merge_route(engine, merge, method):
    """--merge and what the engine offers -> "device" or "host" """
    if merge == "host" or (merge == "auto" and not hasattr(engine, method)):
        return "host"
    if not hasattr(engine, method):
        raise ExpectError("--merge device: the engine has no %s" % method)
    return "device"


def with_merge(merge, route, device_pass, host_pass):
    """the pass on its route; under ``auto`` a negative cell on the device sends the pass to the host, with a line on stderr"""
    if route == "host":
        return host_pass()
    try:
        return device_pass()
    except NegativeCell as e:
        if merge != "auto":
            raise
        fasta.eprint("%s; the pass is run again with the records added up on the host (--merge host)" % e)
        return host_pass()


def new_acc(n_motifs, m):
    from ._lib import NCODE, SITE_LIMBS
    return np.zeros((n_motifs, SITE_LIMBS, m * NCODE), dtype=np.uint64)


def note_bad(first, bad, base):
    """first int64 [n_motifs][2] (indices into the pass, -1: none) takes a batch's verdicts, whose records start at base"""
    new = (first < 0) & (bad >= 0)
    first[new] = bad[new] + base


def merged_result(mid, occ, firsts, sums, ids, windows, not_finite=NOT_FINITE):
    """what the host route makes of a motif's per-record matrices, from what the device route brings home: the checks in the
    host route's order and with its messages.  ``firsts``: per written matrix, in the host route's order, int64 [2] = the
    pass's first record with a non-finite cell and with a negative one; ``sums``: the rounded accumulators"""
    bad = np.flatnonzero(~np.isfinite(occ))
    who = int(bad[0]) if bad.size else next((int(f[0]) for f in firsts if f[0] >= 0), -1)
    if who >= 0:
        raise ExpectError(not_finite % (mid, ids[who]))
    neg = next((int(f[1]) for f in firsts if f[1] >= 0), -1)
    if neg >= 0:
        raise NegativeCell("Motif %s, record %s: an expected count is negative (a cell of the profile is), which the device's "
                           "accumulators cannot hold" % (mid, ids[neg]))
    counted = occ > 0
    if not counted.any():
        raise ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
    if not all(np.isfinite(s).all() for s in sums):
        raise ExpectError("Motif %s: the sum of an expected count over the records is beyond the largest double" % mid)
    ll = math.fsum(math.log2(x) for x in occ[counted].tolist())
    return tuple(sums) + (int(counted.sum()), int((~counted).sum()), int(windows), round(ll, 3))


def run_merged(engine, recs, tables, motif_ids, letters, code_letters, mode, batch_records=BATCH_RECORDS):
    """``run`` with the records added up on the device: per width one long accumulator per motif, batch after batch added into
    it (engine.expect_merged); only the occupancy and the window counts come home per record"""
    from . import _lib, scanner
    n_letters = len(code_letters)
    groups = OrderedDict()
    for mid in motif_ids:
        groups.setdefault(tables[mid].shape[0], []).append(mid)
    out = {}
    for m, mids in groups.items():
        stack = np.stack([tables[mid] for mid in mids])
        acc = new_acc(len(mids), m)
        first = np.full((len(mids), 2), -1, dtype=np.int64)
        occs, wins, ids = [], [], []
        for a in range(0, len(recs), batch_records):
            b = min(len(recs), a + batch_records)
            batch = scanner._RnaBatch(recs[a:b], None if letters == fasta.RNA else letters)
            if len(batch) == 0:
                continue
            stream = pack.Stream(batch.codes, None, batch.offsets, batch.lengths)
            bad, o, w = engine.expect_merged(stream, stack, n_letters, mode, acc)
            note_bad(first, np.asarray(bad), len(ids))
            occs.append(np.asarray(o))
            wins.append(np.asarray(w))
            ids += list(batch.ids)
        E = _lib.site_acc_round(acc).reshape(len(mids), m, -1)[:, :, :n_letters]
        for k, mid in enumerate(mids):
            if not occs:
                raise ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
            out[mid] = merged_result(mid, np.concatenate([o[:, k] for o in occs]), [first[k]], [np.ascontiguousarray(E[k])], ids,
                                     np.concatenate(wins).sum())
    return out


def run(engine, recs, tables, motif_ids, letters, code_letters, mode, batch_records=BATCH_RECORDS, merge="host"):
    """one pass over the records -> {motif id: (E float64 [m][n_letters] in code order, records, skipped, windows, log2
    likelihood)}; tables {motif id: [m][8]}.  One motif group (width) at a time, batch by batch of records.  ``merge``: where
    the records are added up (MERGES); the result does not depend on it."""
    args = (engine, recs, tables, motif_ids, letters, code_letters, mode, batch_records)
    return with_merge(merge, merge_route(engine, merge, "expect_merged"), lambda: run_merged(*args), lambda: run_host(*args))


def run_host(engine, recs, tables, motif_ids, letters, code_letters, mode, batch_records=BATCH_RECORDS):
    """``run`` with every per-record matrix brought home and added up with math.fsum"""
    from . import scanner
    n_letters = len(code_letters)
    groups = OrderedDict()
    for mid in motif_ids:
        groups.setdefault(tables[mid].shape[0], []).append(mid)
    out = {}
    for m, mids in groups.items():
        stack = np.stack([tables[mid] for mid in mids])
        exps, occs, wins, ids = [], [], [], []
        for a in range(0, len(recs), batch_records):
            b = min(len(recs), a + batch_records)
            batch = scanner._RnaBatch(recs[a:b], None if letters == fasta.RNA else letters)
            if len(batch) == 0:
                continue
            stream = pack.Stream(batch.codes, None, batch.offsets, batch.lengths)
            e, o, w = engine.expect(stream, stack, n_letters, mode)
            exps.append(np.asarray(e)[:, :, :, :n_letters])
            occs.append(np.asarray(o))
            wins.append(np.asarray(w))
            ids += list(batch.ids)
        for k, mid in enumerate(mids):
            if not exps:
                raise ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
            occ = np.concatenate([o[:, k] for o in occs])
            cells = [e[:, k] for e in exps]
            bad = np.flatnonzero(~np.isfinite(occ))
            if bad.size == 0:
                bad = np.flatnonzero(~np.isfinite(np.concatenate(cells, axis=0)).all(axis=(1, 2)))
            if bad.size:
                raise ExpectError("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
                                  "(a ratio of the motif is; check the background and the pseudocount)" % (mid, ids[int(bad[0])]))
            counted = occ > 0
            if not counted.any():
                raise ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
            ll = math.fsum(math.log2(x) for x in occ[counted].tolist())
            out[mid] = (fsum_records(cells), int(counted.sum()), int((~counted).sum()), int(np.concatenate(wins).sum()), round(ll, 3))
    return out


def next_odds(E, letters, code_letters, pseudocount, background):
    """the Odds of the next iteration from E [m][n_letters] (code order): what pssm.load_odds makes of E's written file"""
    from . import pssm
    counts = OrderedDict((l, np.ascontiguousarray(E[:, code_letters.index(l)])) for l in letters)
    return pssm.Odds(letters, pssm.odds(pssm.normalize(counts, pseudocount), background))


def pfm_text(results, motif_ids, order, code_letters, library):
    from . import sites
    text = io.StringIO()
    for mid in motif_ids:
        matrix = np.stack([results[mid][:, code_letters.index(l)] for l in order], axis=1)
        if library:
            text.write("#%s\n#" % mid)
        sites._pfm_to(text, order, matrix)
        if library:
            text.write("\n")
    return text.getvalue()


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.expect",
                                     description=("Expected site counts: the letters under every window weighted by the window's "
                                                  "likelihood ratio, one EM step of motif refinement per iteration."))
    parser.add_argument("fasta", metavar="in.fa", help="the sequence FASTA (-p) or structure FASTA (-q)")
    parser.add_argument("-p", "--pfm_seq", dest="pfm_seq", type=str, default=None, help="Sequence PFM")
    parser.add_argument("-q", "--pfm_struct", dest="pfm_struct", type=str, default=None, help="Structure PFM")
    parser.add_argument("-o", "--prefix", dest="prefix", type=str, required=True, help="PREFIX of PREFIX.expected.txt and PREFIX.summary.txt")
    parser.add_argument("-C", "--pseudocount", type=float, dest="pseudocount", default=0, help="Pseudocount for normalizing PFM. [%(default)s]")
    parser.add_argument("-u", "--uniformbg", action="store_true", default=False, dest="uniform_background",
                        help="Use uniform background for the odds ratios [%(default)s]")
    parser.add_argument("-b", "--bg_seq", default=None, dest="bg_seq", help="File of pre-computed background probabilities for sequences")
    parser.add_argument("-B", "--bg_struct", default=None, dest="bg_struct", help="File of pre-computed background probabilities for structures")
    parser.add_argument("--weight", choices=sorted(MODES), default="posterior",
                        help="weight of a window: its likelihood ratio, or that over the record's occupancy [%(default)s]")
    parser.add_argument("--iterations", type=int, default=1, help="EM steps: each takes the last one's expected counts as its PFM [%(default)s]")
    parser.add_argument("--all-motifs", action="store_true", default=False, dest="all_motifs", help="every motif of a multi-PFM file, one call per width [off]")
    parser.add_argument("--struct-format", choices=["auto", "letters", "dotbracket"], default="auto", dest="struct_format",
                        help="-q: what the structure FASTA holds; dot-bracket strings are annotated on the GPU first [%(default)s]")
    parser.add_argument("--batch-records", type=int, default=BATCH_RECORDS, dest="batch_records",
                        help="records per device call; the files do not depend on it [%(default)s]")
    add_merge_option(parser)
    parser.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")
    args = parser.parse_args(argv)
    if args.uniform_background and (args.bg_seq or args.bg_struct):
        parser.error("You cannot set uniform and custom background options at the same time\n")
    if args.batch_records < 1:
        parser.error("--batch-records: must be positive")
    return args


def main(argv=None, engine=None):
    from . import cli, pssm, scanner, sites, store
    from ._lib import MAX_M
    args = getoptions(argv)
    if bool(args.pfm_seq) == bool(args.pfm_struct):
        fasta.eprint("exactly one of -p (sequence PFM) or -q (structure PFM) is required: expected counts of -p with -q pairs are not supported")
        return 1
    if args.iterations < 1:
        fasta.eprint("--iterations: must be at least 1, not %d" % args.iterations)
        return 1
    if os.path.isdir(args.fasta) or store.is_store(args.fasta):
        fasta.eprint("%s is an averaged-structure directory or packed store: expected counts take a FASTA of letters "
                     "(averaged-structure profiles are not supported)" % args.fasta)
        return 1
    seq = bool(args.pfm_seq)
    option, pfm_file = ("-p", args.pfm_seq) if seq else ("-q", args.pfm_struct)
    letters, code_letters = (fasta.RNA, pack.RNA_LETTERS) if seq else (fasta.STRUCT, pack.STRUCT_LETTERS)
    order = sites.SEQ_ORDER if seq else sites.STRUCT_ORDER
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
        summary = ["\t".join(COLUMNS) + "\n"]
        results = None
        for it in range(1, args.iterations + 1):
            tables = dict((mid, odds[mid].ratio_table(code_letters)) for mid in motif_ids)
            got = run(engine, recs, tables, motif_ids, letters, code_letters, MODES[args.weight], args.batch_records, args.merge)
            for mid in motif_ids:
                E, n, skipped, windows, ll = got[mid]
                summary.append("%s\t%d\t%d\t%d\t%d\t%s\n" % (mid, it, n, skipped, windows, repr(ll)))
            results = dict((mid, got[mid][0]) for mid in motif_ids)
            if it < args.iterations:
                odds = dict((mid, next_odds(results[mid], letters, code_letters, args.pseudocount, bg)) for mid in motif_ids)
        text = pfm_text(results, motif_ids, order, code_letters, args.all_motifs)
        with open(args.prefix + ".expected.txt", "w") as out:
            out.write(text)
        with open(args.prefix + ".summary.txt", "w") as out:
            out.write("".join(summary))
        fasta.eprint("Wrote the expected counts of %d motifs after %d iterations" % (len(motif_ids), args.iterations))
        return 0
    except (IOError, ExpectError) as e:
        fasta.eprint(str(e))
        return 1
    finally:
        if own and engine is not None:
            engine.close()


if __name__ == "__main__":
    sys.exit(main())
