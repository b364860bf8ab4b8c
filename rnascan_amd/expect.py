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
from collections import OrderedDict, namedtuple

import numpy as np

from . import fasta, occupancy

COLUMNS = ["Motif_ID", "Iteration", "Records", "Records.Skipped", "Windows", "Log2.Likelihood"]
BATCH_RECORDS = occupancy.BATCH_RECORDS              # records per packed batch (and per device call); the output does not depend on it
MODES = {"ratio": 0, "posterior": 1}                 # _lib.EXPECT_RATIO, _lib.EXPECT_POSTERIOR
MERGES = ("auto", "device", "host")                  # --merge: where the records are added up
NOT_FINITE = ("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
              "(a ratio of the motif is; check the background and the pseudocount)")


class ExpectError(ValueError):
    """what the pass found: said on stderr, exit 1, nothing written"""


class NegativeCell(ExpectError):
    """the device route met a cell < 0, which the long accumulator cannot hold"""


def fsum_records(parts):
    """parts: arrays [n_rec_i][m][n] -> their exact sum over all records, float64 [m][n] (math.fsum per cell)"""
    X = np.concatenate(parts, axis=0)
    out = np.zeros(X.shape[1:], dtype=np.float64)
    for k in range(X.shape[1]):
        for c in range(X.shape[2]):
            out[k, c] = math.fsum(X[:, k, c].tolist())
    return out


def new_acc(n_motifs, m):
    """the long accumulators of n_motifs matrices of m rows (the width; 4 x the width for the letter-pair table of ``expect_pair``)"""
    from ._lib import NCODE, SITE_LIMBS
    return np.zeros((n_motifs, SITE_LIMBS, m * NCODE), dtype=np.uint64)


# ---- one pass over the records, whatever the input form -----------------------------------------------------------------
# An input form (``expect``: one FASTA of letters; ``expect_profile``; ``expect_pair``) describes itself to the pass:
#   motif_ids, groups   the names, and {width: motif indices}
#   order               the motif indices in the order they are finalised (the first that fails is the one named)
#   batches()           a batch source: (ids, stream, cols) per batch (occupancy.letter_batches and its siblings)
#   tables(m, ks, cols) what the engine takes for the motifs ks of width m; made once per width where cols is None
#   host(stream, tables, mode) -> (matrices, occ, windows); merged(stream, tables, mode, accs) -> (bads, occ, windows):
#                       the engine's two methods, their lists in the form's check order; ``method``: the second one's name
#   matrices            a Matrix per matrix: cells kept, None | cols -> the stored column of every written cell, and the matrix
#                       rows per motif column (1; the tables of ``expect_pair --joint`` and ``expect_profile --joint`` have 4)
#   not_finite          the form's message for a non-finite record
Form = namedtuple("Form", "motif_ids groups order batches tables host merged method matrices not_finite")
Matrix = namedtuple("Matrix", "kept stored rows", defaults=(None, 1))


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


class _Accumulator(object):
    """the long accumulators of one matrix and one width on the device route.  The device adds in the batch's stored column
    order.  Where that order can change, the batches of one order share an accumulator, which is folded into the total -- its
    columns mapped to the written cells -- when the order changes and at the end; a matrix whose order never changes
    (``order`` None) is its own total"""

    def __init__(self, n_motifs, m):
        self.n_motifs, self.m = n_motifs, m
        self.total, self.order, self.acc = None, None, new_acc(n_motifs, m)

    def current(self, order):
        if order != self.order:
            self.fold()
            self.order, self.acc = order, new_acc(self.n_motifs, self.m)
        return self.acc

    def fold(self):
        from . import _lib
        if self.order is None:
            return self.acc
        if self.total is None:
            self.total = new_acc(self.n_motifs, self.m)
        cells = self.acc.reshape(self.n_motifs, _lib.SITE_LIMBS, self.m, _lib.NCODE)
        _lib.site_acc_add(self.total, np.ascontiguousarray(cells[:, :, :, self.order + [7]]).reshape(self.total.shape))
        return self.total


def _note_bad(first, bad, base):
    """first int64 [n_motifs][2] (indices into the pass, -1: none) takes a batch's verdicts, whose records start at base"""
    new = (first < 0) & (bad >= 0)
    first[new] = bad[new] + base


def _first_nonfinite(cells):
    """the host route's verdict on one matrix of one motif, as the device gives it: (first record of the pass with a
    non-finite cell, first with a negative one -- which the host route does not look for)"""
    bad = np.flatnonzero(~np.isfinite(np.concatenate(cells, axis=0)).all(axis=(1, 2))) if cells else ()
    return (int(bad[0]) if len(bad) else -1, -1)


def _finalise(mid, not_finite, ids, occs, firsts, sums, windows):
    """a motif's result from what either route brings: its occupancy per batch, per matrix (in the form's check order) the
    first record with a non-finite and with a negative cell, and ``sums()``, the matrices added up over the records ->
    (matrices, records, skipped, windows, log2 likelihood)"""
    occ = np.concatenate(occs) if occs else np.zeros(0)
    bad = np.flatnonzero(~np.isfinite(occ))
    who = int(bad[0]) if bad.size else next((f[0] for f in firsts if f[0] >= 0), -1)
    if who >= 0:
        raise ExpectError(not_finite % (mid, ids[who]))
    neg = next((f[1] for f in firsts if f[1] >= 0), -1)
    if neg >= 0:
        raise NegativeCell("Motif %s, record %s: an expected count is negative (a cell of the profile is), which the device's "
                           "accumulators cannot hold" % (mid, ids[neg]))
    counted = occ > 0
    if not counted.any():
        raise ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
    sums = sums()
    if not all(np.isfinite(s).all() for s in sums):
        raise ExpectError("Motif %s: the sum of an expected count over the records is beyond the largest double" % mid)
    ll = math.fsum(math.log2(x) for x in occ[counted].tolist())
    return sums, int(counted.sum()), int((~counted).sum()), int(windows), round(ll, 3)


def _one_pass(form, mode, device):
    """batches outside, widths inside.  ``device``: the records are added up in long accumulators on the device and only the
    occupancy and the window counts come home per record; else every per-record matrix comes home and math.fsum adds them"""
    from . import _lib
    n_motifs, sides = len(form.motif_ids), range(len(form.matrices))
    occs = [[] for _ in range(n_motifs)]
    wins = dict((m, 0) for m in form.groups)                       # Windows depends on the width
    if device:
        accs = dict((m, [_Accumulator(len(ks), m * mx.rows) for mx in form.matrices]) for m, ks in form.groups.items())
        first = dict((m, [np.full((len(ks), 2), -1, dtype=np.int64) for _ in sides]) for m, ks in form.groups.items())
    else:
        cells = [[[] for _ in sides] for _ in range(n_motifs)]
    made, seen = {}, []
    for ids, stream, cols in form.batches():
        orders = [None if mx.stored is None else mx.stored(cols) for mx in form.matrices]
        for m, ks in form.groups.items():
            tables = made[m] if cols is None and m in made else form.tables(m, ks, cols)
            if cols is None:
                made[m] = tables
            if device:
                bads, o, w = form.merged(stream, tables, mode, [a.current(order) for a, order in zip(accs[m], orders)])
                for f, bad in zip(first[m], bads):
                    _note_bad(f, np.asarray(bad), len(seen))
            else:
                exps, o, w = form.host(stream, tables, mode)
                for i, mx in enumerate(form.matrices):
                    E = np.asarray(exps[i])[:, :, :, :mx.kept] if orders[i] is None else np.asarray(exps[i])[:, :, :, orders[i]]
                    for j, k in enumerate(ks):
                        cells[k][i].append(E[:, j])
            o = np.asarray(o)
            for j, k in enumerate(ks):
                occs[k].append(o[:, j])
            wins[m] += int(np.asarray(w).sum())
        seen += ids
    if device:
        rounded = dict((m, [_lib.site_acc_round(a.fold()).reshape(len(ks), m * mx.rows, -1)[:, :, :mx.kept] for a, mx in zip(accs[m], form.matrices)])
                       for m, ks in form.groups.items())
    place = dict((k, (m, j)) for m, ks in form.groups.items() for j, k in enumerate(ks))
    out = {}
    for k in form.order:
        m, j = place[k]
        if device:
            firsts, sums = [f[j] for f in first[m]], lambda: [np.ascontiguousarray(E[j]) for E in rounded[m]]
        else:
            firsts, sums = [_first_nonfinite(c) for c in cells[k]], lambda: [fsum_records(c) for c in cells[k]]
        out[form.motif_ids[k]] = _finalise(form.motif_ids[k], form.not_finite, seen, occs[k], firsts, sums, wins[m])
    return out


def run(engine, form, mode, merge="host"):
    """one pass over the records -> {motif id: (the expected matrices float64 [m][cells kept], in the form's order; records;
    skipped; windows; log2 likelihood)}.  ``merge``: where the records are added up (MERGES); the result does not depend on it"""
    return with_merge(merge, merge_route(engine, merge, form.method), lambda: _one_pass(form, mode, True), lambda: _one_pass(form, mode, False))


# ---- the iterations and the files of the three commands --------------------------------------------------------------------
# a written matrix: its file's suffix, its slot in a pair (0: sequence, 1: structure), the letters of its cells in the order
# the pass returns them, and the background its PFM is normalised against
Side = namedtuple("Side", "suffix slot code_letters background")


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


def iterate(args, engine, sides, odds, pairs, form_of, what="motifs", more=None):
    """``--iterations`` passes and the files.  ``sides``: the written matrices in the pass's order, which is the files';
    ``odds``: [sequence odds | None, structure odds | None], None where no PFM was given; ``pairs``: [(sequence id | None,
    structure id | None)] into them; ``form_of(odds, pairs)``: the pass's Form.  After a pass every given PFM is replaced by
    its expected matrix -- what reading this iteration's files would give: every motif (pair) under its written name.
    ``more(matrices of the last pass per motif id, motif_ids)`` -> [(suffix, text)]: files of matrices the form has behind the
    sides', which are written and not fed back"""
    from . import sites
    motif_ids = [sites.pair_id(a, b) for a, b in pairs]
    written = ((fasta.RNA, sites.SEQ_ORDER), (fasta.STRUCT, sites.STRUCT_ORDER))
    summary = ["\t".join(COLUMNS) + "\n"]
    for it in range(1, args.iterations + 1):
        got = run(engine, form_of(odds, pairs), MODES[args.weight], args.merge)
        for mid in motif_ids:
            _, n, skipped, windows, ll = got[mid]
            summary.append("%s\t%d\t%d\t%d\t%d\t%s\n" % (mid, it, n, skipped, windows, repr(ll)))
        if it < args.iterations:
            odds = list(odds)
            for i, side in enumerate(sides):
                if odds[side.slot] is not None:
                    odds[side.slot] = OrderedDict((mid, next_odds(got[mid][0][i], written[side.slot][0], side.code_letters, args.pseudocount,
                                                                  side.background)) for mid in motif_ids)
            pairs = [tuple(None if o is None else mid for o in odds) for mid in motif_ids]
    texts = [(side.suffix, pfm_text(dict((mid, got[mid][0][i]) for mid in motif_ids), motif_ids, written[side.slot][1], side.code_letters,
                                    args.all_motifs)) for i, side in enumerate(sides)]
    if more is not None:
        texts += more(dict((mid, got[mid][0]) for mid in motif_ids), motif_ids)
    for suffix, text in texts + [(".summary.txt", "".join(summary))]:
        with open(args.prefix + suffix, "w") as out:
            out.write(text)
    fasta.eprint("Wrote the expected counts of %d %s after %d iterations" % (len(motif_ids), what, args.iterations))


# ---- the options that only the three expect commands have ({words}: occupancy.add_options) ------------------------------------
OPTIONS = dict(occupancy.OPTIONS)
OPTIONS.update({
    "-o": lambda p, w: p.add_argument("-o", "--prefix", dest="prefix", type=str, required=True, help="PREFIX of %s" % w["files"]),
    "--weight": lambda p, w: p.add_argument("--weight", choices=sorted(MODES), default="posterior",
                                            help="weight of a window: its %slikelihood ratio, or that over the record's %soccupancy [%%(default)s]" %
                                                 (w["joint"], w["joint"])),
    "--iterations": lambda p, w: p.add_argument("--iterations", type=int, default=1, help="%s [%%(default)s]" % w["steps"]),
    "--merge": lambda p, w: p.add_argument("--merge", choices=MERGES, default="auto",
                                           help="where the records are added up: exactly on the device (long accumulators), or on the host with "
                                                "math.fsum; the files do not depend on it [%(default)s: device where the engine offers it]"),
})


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.expect",
                                     description=("Expected site counts: the letters under every window weighted by the window's "
                                                  "likelihood ratio, one EM step of motif refinement per iteration."))
    parser.add_argument("fasta", metavar="in.fa", help="the sequence FASTA (-p) or structure FASTA (-q)")
    occupancy.add_options(parser, ["-p", "-q", "-o", "-C", "-u", "-b", "-B", "--weight", "--iterations", "--all-motifs", "--struct-format",
                                   "--batch-records", "--merge", "--device"], OPTIONS, result="files do", joint="",
                          files="PREFIX.expected.txt and PREFIX.summary.txt", steps="EM steps: each takes the last one's expected counts as its PFM")
    args = parser.parse_args(argv)
    occupancy.check_options(parser, args)
    return args


def main(argv=None, engine=None):
    from . import store
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
    with occupancy.Device(engine, args.device, (IOError, ExpectError)) as dev:
        got = occupancy.single_fasta(args, dev)
        if got is None:
            return 1
        motif_ids, letters, code_letters, bg, odds, recs = got
        engine, slot = dev.engine, 0 if args.pfm_seq else 1

        def form_of(odds, pairs):
            mine = [odds[slot][pair[slot]] for pair in pairs]
            groups = occupancy._by_width([o.length for o in mine])

            def host(stream, tables, mode):
                e, o, w = engine.expect(stream, tables, len(code_letters), mode)
                return [e], o, w

            def merged(stream, tables, mode, accs):
                bad, o, w = engine.expect_merged(stream, tables, len(code_letters), mode, accs[0])
                return [bad], o, w
            # the motifs are finalised width by width (widths by first appearance, the file's order within one)
            return Form(motif_ids, groups, [k for ks in groups.values() for k in ks], lambda: occupancy.letter_batches(recs, letters, args.batch_records),
                        lambda m, ks, cols: np.stack([mine[k].ratio_table(code_letters) for k in ks]), host, merged, "expect_merged",
                        [Matrix(len(code_letters))], NOT_FINITE)

        iterate(args, engine, [Side(".expected.txt", slot, code_letters, bg)], [odds, None] if slot == 0 else [None, odds],
                [(mid, None) if slot == 0 else (None, mid) for mid in motif_ids], form_of)
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
