"""Expected site counts of sequence + structure FASTA pairs: one EM step (or several) on both motifs of a pair at once.

    python -m rnascan_amd.expect_pair -p seq.pfm -q struct.pfm [-C c] [-u | -b bg -B bg] [--weight posterior|ratio]
                                      [--iterations N] [--all-motifs] [--struct-format auto|letters|dotbracket]
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

``--iterations N``: both PFMs of a pair are replaced by their expected matrices, normalised with the same pseudocount
against the same backgrounds, and the pass is run again; ``--iterations 2`` writes the bytes of a run on the outputs of a run.

Inputs, pairing, backgrounds and dot-bracket structures are handled exactly as ``occupancy_pair`` handles them (the same
code).  Not supported: the per-column 4 x 7 joint expected table, ``--gpus``, other priors.
"""
import argparse
import math
import sys
from collections import OrderedDict

import numpy as np

from . import expect, fasta, occupancy, occupancy_pair, pack

BATCH_RECORDS = expect.BATCH_RECORDS


NOT_FINITE = ("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
              "(a ratio of one of the motifs is; check the backgrounds and the pseudocount)")


def run(engine, recs, srecs, seq_odds, struct_odds, pairs, mode, batch_records=BATCH_RECORDS, merge="host"):
    """one pass -> {pair id: (E_seq float64 [m][4] in code order, E_struct float64 [m][7] in code order
    (pack.STRUCT_LETTERS), records, skipped, windows, log2 likelihood)}.  ``merge``: where the records are added up
    (expect.MERGES); the result does not depend on it."""
    args = (engine, recs, srecs, seq_odds, struct_odds, pairs, mode, batch_records)
    return expect.with_merge(merge, expect.merge_route(engine, merge, "expect_pair_merged"), lambda: run_merged(*args), lambda: run_host(*args))


def run_merged(engine, recs, srecs, seq_odds, struct_odds, pairs, mode, batch_records=BATCH_RECORDS):
    """``run`` with the records added up on the device (engine.expect_pair_merged): two long accumulators per pair"""
    from . import _lib, sites
    motif_ids = [sites.pair_id(a, b) for a, b in pairs]
    groups = occupancy._by_width([seq_odds[a].length for a, _ in pairs])
    tables = dict((m, occupancy_pair.pair_tables(seq_odds, struct_odds, pairs, ks)) for m, ks in groups.items())
    acc = dict((m, (expect.new_acc(len(ks), m), expect.new_acc(len(ks), m))) for m, ks in groups.items())
    first = dict((m, (np.full((len(ks), 2), -1, dtype=np.int64), np.full((len(ks), 2), -1, dtype=np.int64))) for m, ks in groups.items())
    occs = dict((k, []) for k in range(len(pairs)))
    wins = dict((m, 0) for m in groups)                            # Windows depends on the width
    seen = []
    for ids, stream in occupancy_pair.batches(recs, srecs, batch_records):
        for m, ks in groups.items():
            bq, bs, o, w = engine.expect_pair_merged(stream, tables[m][0], tables[m][1], mode, acc[m][0], acc[m][1])
            expect.note_bad(first[m][0], np.asarray(bq), len(seen))
            expect.note_bad(first[m][1], np.asarray(bs), len(seen))
            o = np.asarray(o)
            for j, k in enumerate(ks):
                occs[k].append(o[:, j])
            wins[m] += int(np.asarray(w).sum())
        seen += ids
    out = {}
    place = dict((k, (m, j)) for m, ks in groups.items() for j, k in enumerate(ks))
    sums = dict((m, (_lib.site_acc_round(acc[m][0]).reshape(len(ks), m, -1)[:, :, :4], _lib.site_acc_round(acc[m][1]).reshape(len(ks), m, -1)[:, :, :7]))
                for m, ks in groups.items())
    for k, mid in enumerate(motif_ids):
        if not occs[k]:
            raise expect.ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
        m, j = place[k]
        out[mid] = expect.merged_result(mid, np.concatenate(occs[k]), [first[m][0][j], first[m][1][j]],
                                        [np.ascontiguousarray(sums[m][0][j]), np.ascontiguousarray(sums[m][1][j])], seen, wins[m], NOT_FINITE)
    return out


def run_host(engine, recs, srecs, seq_odds, struct_odds, pairs, mode, batch_records=BATCH_RECORDS):
    """``run`` with every per-record matrix brought home and added up with math.fsum"""
    from . import sites
    motif_ids = [sites.pair_id(a, b) for a, b in pairs]
    groups = occupancy._by_width([seq_odds[a].length for a, _ in pairs])
    tables = dict((m, occupancy_pair.pair_tables(seq_odds, struct_odds, pairs, ks)) for m, ks in groups.items())
    esq = dict((k, []) for k in range(len(pairs)))
    est = dict((k, []) for k in range(len(pairs)))
    occs = dict((k, []) for k in range(len(pairs)))
    wins = dict((k, []) for k in range(len(pairs)))                # Windows depends on the width
    seen = []
    for ids, stream in occupancy_pair.batches(recs, srecs, batch_records):
        for m, ks in groups.items():
            eq, es, o, w = engine.expect_pair(stream, tables[m][0], tables[m][1], mode)
            eq, es, o = np.asarray(eq), np.asarray(es), np.asarray(o)
            for j, k in enumerate(ks):
                esq[k].append(eq[:, j, :, :4])
                est[k].append(es[:, j, :, :7])
                occs[k].append(o[:, j])
                wins[k].append(np.asarray(w))
        seen += ids
    out = {}
    for k, mid in enumerate(motif_ids):
        if not occs[k]:
            raise expect.ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
        occ = np.concatenate(occs[k])
        bad = np.flatnonzero(~np.isfinite(occ))
        for cells in (esq[k], est[k]):
            if bad.size == 0:
                bad = np.flatnonzero(~np.isfinite(np.concatenate(cells, axis=0)).all(axis=(1, 2)))
        if bad.size:
            raise expect.ExpectError("Motif %s, record %s: the occupancy or an expected count is infinite or not a number "
                                     "(a ratio of one of the motifs is; check the backgrounds and the pseudocount)" % (mid, seen[int(bad[0])]))
        counted = occ > 0
        if not counted.any():
            raise expect.ExpectError("Motif %s: no record contributes (every occupancy is 0)" % mid)
        ll = math.fsum(math.log2(x) for x in occ[counted].tolist())
        out[mid] = (expect.fsum_records(esq[k]), expect.fsum_records(est[k]), int(counted.sum()), int((~counted).sum()),
                    int(np.concatenate(wins[k]).sum()), round(ll, 3))
    return out


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.expect_pair",
                                     description=("Expected site counts of sequence + structure FASTA pairs: the letters of both files "
                                                  "under every window, weighted by the window's joint likelihood ratio."))
    occupancy_pair.add_options(parser)
    parser.add_argument("-o", "--prefix", dest="prefix", type=str, required=True,
                        help="PREFIX of PREFIX.expected.seq.txt, PREFIX.expected.struct.txt and PREFIX.summary.txt")
    parser.add_argument("--weight", choices=sorted(expect.MODES), default="posterior",
                        help="weight of a window: its joint likelihood ratio, or that over the record's joint occupancy [%(default)s]")
    parser.add_argument("--iterations", type=int, default=1, help="EM steps: each takes the last one's expected matrices as its PFMs [%(default)s]")
    expect.add_merge_option(parser)
    args = parser.parse_intermixed_args(argv)
    occupancy_pair.check_options(parser, args)
    args.single, args.profiles = "expect", "expect_profile"
    return args


def main(argv=None, engine=None):
    from . import scanner, sites
    args = getoptions(argv)
    if args.iterations < 1:
        fasta.eprint("--iterations: must be at least 1, not %d" % args.iterations)
        return 1
    checked = occupancy_pair.check_inputs(args)
    if checked is None:
        return 1
    pairs = checked[0]
    own = engine is None
    struct_letters = list(pack.STRUCT_LETTERS)
    try:
        if engine is None:
            engine = scanner.HipEngine(args.device)
        recs, srecs, seq_odds, struct_odds, bg_seq, bg_struct = occupancy_pair.sources(args, engine)
        motif_ids = [sites.pair_id(a, b) for a, b in pairs]
        summary = ["\t".join(expect.COLUMNS) + "\n"]
        got = None
        for it in range(1, args.iterations + 1):
            got = run(engine, recs, srecs, seq_odds, struct_odds, pairs, expect.MODES[args.weight], args.batch_records, args.merge)
            for mid in motif_ids:
                _, _, n, skipped, windows, ll = got[mid]
                summary.append("%s\t%d\t%d\t%d\t%d\t%s\n" % (mid, it, n, skipped, windows, repr(ll)))
            if it < args.iterations:
                # what reading this iteration's files would give: every pair under its written name
                seq_odds = OrderedDict((mid, expect.next_odds(got[mid][0], fasta.RNA, pack.RNA_LETTERS, args.pseudocount, bg_seq)) for mid in motif_ids)
                struct_odds = OrderedDict((mid, expect.next_odds(got[mid][1], fasta.STRUCT, struct_letters, args.pseudocount, bg_struct))
                                          for mid in motif_ids)
                pairs = [(mid, mid) for mid in motif_ids]
        texts = [(".expected.seq.txt", expect.pfm_text(dict((mid, got[mid][0]) for mid in motif_ids), motif_ids, sites.SEQ_ORDER,
                                                        pack.RNA_LETTERS, args.all_motifs)),
                 (".expected.struct.txt", expect.pfm_text(dict((mid, got[mid][1]) for mid in motif_ids), motif_ids, sites.STRUCT_ORDER,
                                                           struct_letters, args.all_motifs)),
                 (".summary.txt", "".join(summary))]
        for suffix, text in texts:
            with open(args.prefix + suffix, "w") as out:
                out.write(text)
        fasta.eprint("Wrote the expected counts of %d motif pairs after %d iterations" % (len(motif_ids), args.iterations))
        return 0
    except (IOError, expect.ExpectError, sites.InputError) as e:
        fasta.eprint(str(e))
        return 1
    finally:
        if own and engine is not None:
            engine.close()


if __name__ == "__main__":
    sys.exit(main())
