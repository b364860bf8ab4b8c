"""In-silico mutagenesis: which single-nucleotide changes create or destroy a site of a motif.

    python -m rnascan_amd.variants -p seq.pfm [-C c] [-m M] [-u | -b bg] [--all-motifs] [--effects-only] [--device D]
                                   (--variants FILE | --saturate) seqs.fa > table.tsv

The PSSM is built exactly as ``rnascan -p`` builds it.  For a position p of a record and a letter a, the score that
counts is the best window over p if p held a: the greatest float32 score among the windows of the record
that cover p, the lowest start on a tie; the column of the letter the record holds there is the unmutated best ("ref").
At the threshold -m a change is a ``gain`` (the alt best passes, the ref best does not), a ``loss`` (the reverse),
``kept`` (both pass) or ``none``; compares are strict, as ``rnascan``'s ``score > minscore``.

``--variants FILE``: tab-separated ``Seq_ID  Pos  Ref  Alt`` (an optional header line starting with ``Seq_ID``); ``Pos``
is 1-based in the record as ``Start`` is, ``Ref`` / ``Alt`` one letter of ACGTU in either case, T = U.  One row per
variant (input order) x motif (file order); ``--effects-only`` drops the ``kept`` and ``none`` rows.
``--saturate``: every position x the three other letters; only ``gain`` and ``loss`` rows, ordered by record, Pos, Alt in
ACGU order, then motif.  Only the events leave the device (``HipEngine.mutmap_events``); their window starts come from
``HipEngine.variants`` on the events.

Columns: Motif_ID Seq_ID Pos Ref Alt Ref.Start Ref.LogOdds Alt.Start Alt.LogOdds Delta Effect -- starts 1-based, LogOdds as
the scan prints it (``np.round`` of the float32 to 3 places), Delta = float64(alt) - float64(ref) of the unrounded scores
rounded the same way, empty when it is not a number (a side without any window).  The bytes do not depend on how the
records are batched.  Insertions and deletions are not supported; the structure side is not touched by a letter change
without refolding and stays outside this tool.
"""
import argparse
import os
import sys

import numpy as np

from . import fasta, pack

COLUMNS = ["Motif_ID", "Seq_ID", "Pos", "Ref", "Alt", "Ref.Start", "Ref.LogOdds", "Alt.Start", "Alt.LogOdds", "Delta", "Effect"]
EFFECTS = ("none", "gain", "loss", "kept")          # index = (alt passes) + 2 * (ref passes)
BATCH_RECORDS = 4096                                 # records per packed batch (and per device call); the output does not depend on it
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


class VariantsError(ValueError):
    """a line of the variants file that cannot be used; ``line`` is its 1-based number in the file"""

    def __init__(self, path, line, msg):
        ValueError.__init__(self, "%s, line %d: %s" % (path, line, msg))
        self.line = line


def _allele(path, line, what, text):
    if len(text) != 1:
        raise VariantsError(path, line, "%s %r is not a single letter: indels are not supported" % (what, text))
    code = _CODE.get(text.upper())
    if code is None:
        raise VariantsError(path, line, "%s %r is not a nucleotide (one of ACGTU)" % (what, text))
    return code


def parse_variants(path, lines=None):
    """-> [(line number, Seq_ID, 0-based position in the record, ref code, alt code)] in file order"""
    if lines is None:
        with open(path, "r") as f:
            lines = f.read().splitlines()
    out = []
    for no, raw in enumerate(lines, 1):
        text = raw.rstrip("\r\n")
        if not text.strip() or text.startswith("#"):
            continue
        if not out and text.startswith("Seq_ID"):
            continue
        fields = text.split("\t")
        if len(fields) < 4:
            raise VariantsError(path, no, "expected four tab-separated fields Seq_ID, Pos, Ref, Alt, found %d" % len(fields))
        sid, pos, ref, alt = (f.strip() for f in fields[:4])
        try:
            p = int(pos)
        except ValueError:
            raise VariantsError(path, no, "Pos %r is not an integer" % pos)
        out.append((no, sid, p - 1, _allele(path, no, "Ref", ref), _allele(path, no, "Alt", alt)))
    return out


def resolve(path, variants, ids, lengths):
    """checks ids and positions -> (record index int64 [n], start int64 [n]) in file order"""
    index = {}
    for k, sid in enumerate(ids):
        index.setdefault(sid, k)
    rec = np.empty(len(variants), dtype=np.int64)
    start = np.empty(len(variants), dtype=np.int64)
    for i, (no, sid, p, _, _) in enumerate(variants):
        if sid not in index:
            raise VariantsError(path, no, "unknown Seq_ID %r" % sid)
        r = index[sid]
        if not (0 <= p < int(lengths[r])):
            raise VariantsError(path, no, "Pos %d lies outside record %s (%d letters)" % (p + 1, sid, int(lengths[r])))
        rec[i], start[i] = r, p
    return rec, start


def classify(ref, alt, thr):
    """effect index (into EFFECTS) per entry: strict compares of the float32 scores with thr; NaN and -inf never pass"""
    with np.errstate(invalid="ignore"):
        pr = np.asarray(ref, dtype=np.float32).astype(np.float64) > float(thr)
        pa = np.asarray(alt, dtype=np.float32).astype(np.float64) > float(thr)
    return pa.astype(np.int64) + 2 * pr.astype(np.int64)


def _starts(pos1, where):
    """1-based window starts as strings, empty where there is no window"""
    s = np.asarray(pos1, dtype=np.int64) - np.asarray(where, dtype=np.int64)
    return [str(int(x)) if w >= 0 else "" for x, w in zip(s.tolist(), np.asarray(where).tolist())]


def rows(motif_ids, seq_ids, pos1, ref_code, alt_code, ref, alt, ref_where, alt_where, thr):
    """the table's columns for n entries (lists / arrays of one length) -> (ordered dict of columns, effect index)"""
    ref = np.asarray(ref, dtype=np.float32)
    alt = np.asarray(alt, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        delta = np.round(alt.astype(np.float64) - ref.astype(np.float64), 3)
    eff = classify(ref, alt, thr)
    cols = {"Motif_ID": list(motif_ids), "Seq_ID": list(seq_ids), "Pos": np.asarray(pos1, dtype=np.int64),
            "Ref": [pack.RNA_LETTERS[c] for c in np.asarray(ref_code).tolist()],
            "Alt": [pack.RNA_LETTERS[c] for c in np.asarray(alt_code).tolist()],
            "Ref.Start": _starts(pos1, ref_where), "Ref.LogOdds": np.round(ref, 3),
            "Alt.Start": _starts(pos1, alt_where), "Alt.LogOdds": np.round(alt, 3),
            "Delta": delta, "Effect": [EFFECTS[e] for e in eff.tolist()]}
    return cols, eff


def _keep(cols, keep):
    keep = np.flatnonzero(keep)
    return dict((k, ([v[i] for i in keep.tolist()] if isinstance(v, list) else v[keep])) for k, v in cols.items()), int(keep.size)


def _by_width(pssm, motif_ids):
    groups = {}
    for k, mid in enumerate(motif_ids):
        groups.setdefault(pssm[mid].length, []).append(k)
    return groups


def run_list(engine, writer, recs, pssm, motif_ids, path, variants, thr, effects_only=False):
    """--variants: rows in (variant, motif) order, batch by batch of records; every file error is raised before a row is written"""
    from . import scanner
    from ._lib import MAX_M
    ids, lengths = list(recs.ids), np.asarray(recs.lengths, dtype=np.int64)
    rec, start = resolve(path, variants, ids, lengths)
    ref_code = np.asarray([v[3] for v in variants], dtype=np.uint8)
    alt_code = np.asarray([v[4] for v in variants], dtype=np.uint8)
    n_var, n_mo = len(variants), len(motif_ids)
    for mid in motif_ids:
        if pssm[mid].length > MAX_M:
            raise ValueError("motif %s is %d positions wide, more than %d (PFMSCAN_MAX_M)" % (mid, pssm[mid].length, MAX_M))
    ref = np.full((n_var, n_mo), np.nan, dtype=np.float32)
    alt = np.full((n_var, n_mo), np.nan, dtype=np.float32)
    rw = np.full((n_var, n_mo), -1, dtype=np.int8)
    aw = np.full((n_var, n_mo), -1, dtype=np.int8)
    groups = _by_width(pssm, motif_ids)
    for a in range(0, len(ids), BATCH_RECORDS):
        b = min(len(ids), a + BATCH_RECORDS)
        mine = np.flatnonzero((rec >= a) & (rec < b))
        if mine.size == 0:
            continue
        batch = scanner._RnaBatch(recs[a:b])
        stream = pack.Stream(batch.codes, None, batch.offsets, batch.lengths)
        pos = batch.offsets[rec[mine] - a] + start[mine]
        bad = np.flatnonzero(batch.codes[pos] != ref_code[mine])
        if bad.size:
            i = int(mine[bad[0]])
            c = int(batch.codes[pos[bad[0]]])
            raise VariantsError(path, variants[i][0], "Ref %s is not the letter of record %s at Pos %d (%s)" %
                                (pack.RNA_LETTERS[ref_code[i]], variants[i][1], variants[i][2] + 1, pack.RNA_LETTERS[c] if c < 4 else "not a nucleotide"))
        for m, ks in groups.items():
            T = np.stack([pssm[motif_ids[k]].letter_table(pack.RNA_LETTERS) for k in ks])
            r, al, w1, w2 = engine.variants(stream, T, pos, alt_code[mine])
            ref[np.ix_(mine, ks)], alt[np.ix_(mine, ks)], rw[np.ix_(mine, ks)], aw[np.ix_(mine, ks)] = r, al, w1, w2
    v = np.repeat(np.arange(n_var), n_mo)
    q = np.tile(np.arange(n_mo), n_var)
    cols, eff = rows([motif_ids[k] for k in q.tolist()], [variants[i][1] for i in v.tolist()], start[v] + 1, ref_code[v], alt_code[v],
                     ref.reshape(-1), alt.reshape(-1), rw.reshape(-1), aw.reshape(-1), thr)
    n = v.size
    if effects_only:
        cols, n = _keep(cols, (eff == 1) | (eff == 2))
    writer.write_chunk(cols, n)
    return n


def run_saturate(engine, writer, recs, pssm, motif_ids, thr):
    """--saturate: the gain / loss events of every record, position and other letter, batch by batch"""
    from . import scanner
    from ._lib import MAX_M
    ids = list(recs.ids)
    for mid in motif_ids:
        if pssm[mid].length > MAX_M:
            raise ValueError("motif %s is %d positions wide, more than %d (PFMSCAN_MAX_M)" % (mid, pssm[mid].length, MAX_M))
    tables = [pssm[mid].letter_table(pack.RNA_LETTERS) for mid in motif_ids]
    total = 0
    for a in range(0, len(ids), BATCH_RECORDS):
        b = min(len(ids), a + BATCH_RECORDS)
        batch = scanner._RnaBatch(recs[a:b])
        stream = pack.Stream(batch.codes, None, batch.offsets, batch.lengths)
        keys, mos, refs, alts, rws, aws = [], [], [], [], [], []
        for k, T in enumerate(tables):
            key, r, al = engine.mutmap_events(stream, T, thr)
            if key.size == 0:
                continue
            # the events' window starts: the variants kernel on the events alone (the same scores again)
            r2, al2, w1, w2 = engine.variants(stream, T[None], key >> 2, (key & 3).astype(np.uint8))
            if not (np.array_equal(r2[:, 0].view(np.uint32), r.view(np.uint32)) and np.array_equal(al2[:, 0].view(np.uint32), al.view(np.uint32))):
                raise RuntimeError("the variants kernel and the map disagree on the scores of an event")
            keys.append(key)
            mos.append(np.full(key.size, k, dtype=np.int64))
            refs.append(r)
            alts.append(al)
            rws.append(w1[:, 0])
            aws.append(w2[:, 0])
        if not keys:
            continue
        key, mo = np.concatenate(keys), np.concatenate(mos)
        order = np.lexsort((mo, key))
        key, mo = key[order], mo[order]
        pos = key >> 2
        rec, start = stream.locate(pos)
        cols, _ = rows([motif_ids[k] for k in mo.tolist()], [batch.ids[i] for i in rec.tolist()], start + 1, batch.codes[pos], key & 3,
                       np.concatenate(refs)[order], np.concatenate(alts)[order], np.concatenate(rws)[order], np.concatenate(aws)[order], thr)
        writer.write_chunk(cols, key.size)
        total += int(key.size)
    return total


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.variants",
                                     description=("In-silico mutagenesis: the single-nucleotide changes that create or destroy a site of "
                                                  "a sequence motif, for a list of variants or for every position of the records."))
    parser.add_argument("fasta", metavar="seqs.fa", help="the sequence FASTA")
    parser.add_argument("-p", "--pfm_seq", dest="pfm_seq", type=str, required=True, help="Sequence PFM (the first motif of a multi-PFM file; every motif with --all-motifs)")
    parser.add_argument("-C", "--pseudocount", type=float, dest="pseudocount", default=0, help="Pseudocount for normalizing PFM. [%(default)s]")
    parser.add_argument("-m", "--minscore", type=float, dest="minscore", default=6, help="Threshold a site must exceed, as rnascan's. [%(default)s]")
    parser.add_argument("-u", "--uniformbg", action="store_true", default=False, dest="uniform_background",
                        help="Use uniform background for calculating log-odds [%(default)s]")
    parser.add_argument("-b", "--bg_seq", default=None, dest="bg_seq", help="File of pre-computed background probabilities for sequences")
    parser.add_argument("--all-motifs", action="store_true", default=False, dest="all_motifs", help="every motif of a multi-PFM file, one call per width [off]")
    parser.add_argument("--effects-only", action="store_true", default=False, dest="effects_only", help="with --variants: only the gain and loss rows [off]")
    parser.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")
    mode = parser.add_mutually_exclusive_group(required=True)
    mode.add_argument("--variants", dest="variants", metavar="FILE", help="tab-separated Seq_ID, Pos (1-based), Ref, Alt")
    mode.add_argument("--saturate", action="store_true", default=False, help="every position x the three other letters; gain and loss rows only")
    args = parser.parse_args(argv)
    if args.uniform_background and args.bg_seq:
        parser.error("You cannot set uniform and custom background options at the same time\n")
    if args.minscore != args.minscore:
        parser.error("-m: not a number")
    return args


def main(argv=None, engine=None, out=None):
    from . import cli, scanner, table
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    own = engine is None
    try:
        variants = parse_variants(args.variants) if args.variants else None
        bg = fasta.load_background(args.bg_seq, args.uniform_background, args.fasta, fasta.RNA, True)
        pssm = cli.load_motif(args.pfm_seq, args.pseudocount, fasta.RNA, bg)
        if not pssm:
            fasta.eprint("No motif could be read from %s" % args.pfm_seq)
            return 1
        motif_ids = list(pssm.keys()) if args.all_motifs else [scanner._first_motif(pssm)[0]]
        recs = fasta.open_lazy(args.fasta)
        if engine is None:
            engine = scanner.HipEngine(args.device)
        writer = table.TsvWriter(out, COLUMNS, match_id=False)
        if variants is not None:
            n = run_list(engine, writer, recs, pssm, motif_ids, args.variants, variants, float(args.minscore), args.effects_only)
        else:
            n = run_saturate(engine, writer, recs, pssm, motif_ids, float(args.minscore))
        writer.close()
        out.flush()
        fasta.eprint("Wrote %d rows" % n)
        return 0
    except (VariantsError, IOError) as e:
        fasta.eprint(str(e))
        return 1
    finally:
        if own and engine is not None:
            engine.close()


if __name__ == "__main__":
    sys.exit(main())
