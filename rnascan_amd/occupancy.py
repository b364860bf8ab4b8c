"""Occupancy: how much of each motif does each record carry -- a records x motifs table, no threshold.

    python -m rnascan_amd.occupancy (-p seq.pfm | -q struct.pfm) [-C c] [-u | -b bg | -B bg] [--all-motifs]
                                    [--struct-format auto|letters|dotbracket] [--device N] in.fa > table.tsv
    python -m rnascan_amd.occupancy -q struct.pfm [...] avgdir_or_store/ > table.tsv
    python -m rnascan_amd.occupancy -p seq.pfm -q struct.pfm [...] seqs.fa avgdir_or_store/ > table.tsv

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

Averaged-structure profiles (a directory of ``structure.<id>.txt`` files or a packed store as the last input):
the structure part of a window's ratio is the product over its rows of the marginal ratio sum_c r[c] * R[c] -- the expected
odds of the row, not 2 ** (expected log-odds), which is what a structure scan's score would give.  ``-q`` alone: structure
only, every window inside a record has a term.  ``-p`` with ``-q``: the sequence ratio of the FASTA's record times the
structure marginals of its profile, the ratio behind ``LogOdds.SeqStruct``; records and profiles are matched by id, the
motifs of two libraries are paired as ``rnascan`` pairs them (``Motif_ID`` as the site profiles name a pair).  The
structure background is ``-u``, ``-B file``, or else computed from the profiles as ``rnascan`` computes it; ``--pairing``
pairs the profile's columns with the PFM's as ``rnascan`` does, ``--profile-dtype`` is the rows' storage on the device (the
store's own, or float64 for text files, unless given).  Two-FASTA pairs (``-p -q seqs.fa structs.fa``) are refused here: they are
``python -m rnascan_amd.occupancy_pair``.
"""
import argparse
import math
from collections import OrderedDict
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


def _by_width(widths):
    groups = {}
    for k, m in enumerate(widths):
        groups.setdefault(m, []).append(k)
    return groups


# ---- the batch sources: generators of (ids, pack.Stream, cols); the third is ``occupancy_pair.batches`` ---------------------
def letter_batches(recs, letters, batch_records=BATCH_RECORDS):
    """a letters FASTA, batch by batch of records: every batch that holds a record; ``cols`` is None"""
    from . import scanner
    for a in range(0, len(recs), batch_records):
        b = min(len(recs), a + batch_records)
        batch = scanner._RnaBatch(recs[a:b], None if letters == fasta.RNA else letters)
        if len(batch) == 0:
            continue
        yield list(batch.ids), pack.Stream(batch.codes, None, batch.offsets, batch.lengths), None


def profile_batches(recs, profiles, batch_records=BATCH_RECORDS):
    """an averaged-structure input (``sites._Profiles``), batch by batch of records and within a batch run by run of equal
    column order: ``cols`` is the run's stored order.  ``recs``: the FASTA's records in the profiles' order (their codes go
    beside the rows), or None (structure only)"""
    for a in range(0, len(profiles.ids), batch_records):
        b = min(len(profiles.ids), a + batch_records)
        at = a
        for ids, cols, pst in profiles.runs(a, b):
            yield list(ids), paired_batch(recs, at, ids, pst), cols
            at += len(ids)


def profile_tables(seq_odds, struct_odds, pairs, pairing="aligned"):
    """-> tables(m, ks, cols) = (structure tables of the pairs ks in the stored column order cols | None, their sequence
    tables | None); ``pairs``: [(sequence id | None, structure id | None)], all of one kind"""
    from . import scanner
    seq_tables = {}

    def tables(m, ks, cols):
        if pairs[0][0] is not None and m not in seq_tables:
            seq_tables[m] = np.stack([seq_odds[pairs[k][0]].ratio_table(pack.RNA_LETTERS) for k in ks])
        # the structure tables in THIS run's stored column order
        st = np.stack([scanner.struct_matrix(struct_odds[pairs[k][1]], cols, pairing) for k in ks]) if pairs[0][1] is not None else None
        return st, seq_tables.get(m)
    return tables


def write_table(out, motif_ids, groups, batches, call):
    """the table: the header, then rows in (record, motif) order, batch by batch; one device call per batch and width.
    ``groups``: {width: motif indices}; ``call(stream, m, ks, cols)`` -> (occ [n_rec][len(ks)], windows [n_rec])"""
    out.write("\t".join(COLUMNS) + "\n")
    total = 0
    for ids, stream, cols in batches:
        occ = np.zeros((len(ids), len(motif_ids)), dtype=np.float64)
        win = np.zeros((len(ids), len(motif_ids)), dtype=np.int64)
        for m, ks in groups.items():
            o, w = call(stream, m, ks, cols)
            occ[:, ks] = o
            win[:, ks] = np.asarray(w)[:, None]
        out.write("".join(format_rows(motif_ids, ids, win, occ)))
        total += len(ids) * len(motif_ids)
    out.flush()
    fasta.eprint("Wrote %d rows" % total)


# ---- the options of the five commands of the family, each declared once; {words} differ between the commands ---------------
OPTIONS = {
    "-p": lambda p, w: p.add_argument("-p", "--pfm_seq", dest="pfm_seq", type=str, default=None, help="Sequence PFM"),
    "-q": lambda p, w: p.add_argument("-q", "--pfm_struct", dest="pfm_struct", type=str, default=None, help="Structure PFM"),
    "-C": lambda p, w: p.add_argument("-C", "--pseudocount", type=float, dest="pseudocount", default=0, help="Pseudocount for normalizing PFM. [%(default)s]"),
    "-u": lambda p, w: p.add_argument("-u", "--uniformbg", action="store_true", default=False, dest="uniform_background",
                                      help="Use uniform background for the odds ratios [%(default)s]"),
    "-b": lambda p, w: p.add_argument("-b", "--bg_seq", default=None, dest="bg_seq", help="File of pre-computed background probabilities for sequences"),
    "-B": lambda p, w: p.add_argument("-B", "--bg_struct", default=None, dest="bg_struct", help="File of pre-computed background probabilities for structures"),
    "--all-motifs": lambda p, w: p.add_argument("--all-motifs", action="store_true", default=False, dest="all_motifs",
                                                help="every %s, one call per width [off]" % w["every"]),
    "--struct-format": lambda p, w: p.add_argument("--struct-format", choices=["auto", "letters", "dotbracket"], default="auto", dest="struct_format",
                                                   help="%swhat the structure FASTA holds; dot-bracket strings are annotated on the GPU first [%%(default)s]" % w["q"]),
    "--batch-records": lambda p, w: p.add_argument("--batch-records", type=int, default=BATCH_RECORDS, dest="batch_records",
                                                   help="records per device call; the %s not depend on it [%%(default)s]" % w["result"]),
    "--pairing": lambda p, w: p.add_argument("--pairing", choices=["aligned", "positional"], default="aligned",
                                             help="averaged-structure columns vs structure PFM, as rnascan's [%(default)s]"),
    "--profile-dtype": lambda p, w: p.add_argument("--profile-dtype", choices=["float32", "float64"], default=None, dest="profile_dtype",
                                                   help="device storage of averaged-structure rows [the store's own dtype; float64 for text files]"),
    "--device": lambda p, w: p.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]"),
}
WORDS = {"every": "motif of a multi-PFM file", "q": "-q: ", "result": "table does"}


def add_options(parser, names, options=OPTIONS, **words):
    """declare the options ``names`` in this order, the one the command's --help lists them in"""
    for name in names:
        options[name](parser, dict(WORDS, **words))


def check_options(parser, args):
    if args.uniform_background and (args.bg_seq or args.bg_struct):
        parser.error("You cannot set uniform and custom background options at the same time\n")
    if args.batch_records < 1:
        parser.error("--batch-records: must be positive")


def getoptions(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.occupancy",
                                     description=("Occupancy: the summed likelihood ratio of every record under every motif, "
                                                  "a threshold-free records x motifs table."))
    parser.add_argument("inputs", metavar="input", nargs="+",
                        help=("the sequence FASTA (-p) or structure FASTA (-q); or an averaged-structure directory or packed store (-q); "
                              "or the sequence FASTA and the averaged-structure directory or store (-p with -q)"))
    add_options(parser, ["-p", "-q", "-C", "-u", "-b", "-B", "--all-motifs", "--struct-format", "--batch-records", "--pairing", "--profile-dtype",
                         "--device"])
    args = parser.parse_intermixed_args(argv)                      # `seqs.fa --batch-records 64 avgdir/` is fine
    check_options(parser, args)
    if len(args.inputs) > 2:
        parser.error("one input, or the sequence FASTA and the averaged-structure directory or store")
    args.fasta = args.inputs[0]
    return args


class Device(object):
    """the engine of a command's ``main``: the caller's, or a HipEngine opened when ``engine`` is first asked for and closed
    on the way out.  As a context manager it says an exception of the types ``caught`` on stderr and swallows it: the
    command then returns 1"""

    def __init__(self, engine, device, caught):
        self._engine, self._own, self._device, self._caught = engine, engine is None, device, caught

    @property
    def engine(self):
        if self._engine is None:
            from . import scanner
            self._engine = scanner.HipEngine(self._device)
        return self._engine

    def __enter__(self):
        return self

    def __exit__(self, kind, error, trace):
        said = kind is not None and issubclass(kind, self._caught)
        if said:
            fasta.eprint(str(error))
        if self._own and self._engine is not None:
            self._engine.close()
        return said


def _is_profiles(path):
    from . import store
    return os.path.isdir(path) or store.is_store(path)


def _widths_ok(shapes, motif_ids, option, pfm_file):
    from ._lib import MAX_M
    for mid in motif_ids:
        if shapes[mid].length > MAX_M:
            fasta.eprint("%s: motif %s of %s is %d positions wide, more than %d (PFMSCAN_MAX_M)" %
                         (option, mid, pfm_file, shapes[mid].length, MAX_M))
            return False
    return True


def _load_shapes(pfm_file, option, pseudocount, letters):
    """widths only, before any device work -> {id: Odds} or None (said on stderr)"""
    from . import pssm
    try:
        shapes = pssm.load_odds(pfm_file, pseudocount, letters, None)
    except KeyError:
        fasta.eprint("Failed to load motif %s (%s): check that the PFM has the letters %s" % (pfm_file, option, letters))
        return None
    if not shapes:
        fasta.eprint("No motif could be read from %s (%s)" % (pfm_file, option))
        return None
    return shapes


def profile_motifs(args):
    """the motifs of an averaged-structure run, before any device work: -> (pairs, st_shapes, seq_shapes) or None (said on
    stderr).  ``-q`` alone: pairs [(None, structure id)]; ``-p`` with ``-q``: [(sequence id, structure id)] as ``rnascan``
    pairs two libraries, pairs of unequal width an error; ``-p`` alone (``expect_profile``): [(sequence id, None)].  Shared
    with ``expect_profile``."""
    from . import scanner, sites
    joint = bool(args.pfm_seq) and bool(args.pfm_struct)
    st_shapes = seq_shapes = None
    if args.pfm_struct:
        st_shapes = _load_shapes(args.pfm_struct, "-q", args.pseudocount, fasta.STRUCT)
        if st_shapes is None:
            return None
    if args.pfm_seq:
        seq_shapes = _load_shapes(args.pfm_seq, "-p", args.pseudocount, fasta.RNA)
        if seq_shapes is None:
            return None
    if not args.all_motifs:
        st_shapes = OrderedDict([scanner._first_motif(st_shapes)]) if st_shapes is not None else None
        seq_shapes = OrderedDict([scanner._first_motif(seq_shapes)]) if seq_shapes is not None else None
    if joint:
        try:
            pairs = sites.motif_pairs(seq_shapes, st_shapes)
        except sites.InputError as e:
            fasta.eprint(str(e))
            return None
        # scanner.pair_motifs leaves out the pairs of unequal width (they share no window): here that is an error
        sk, tk = list(seq_shapes.keys()), list(st_shapes.keys())
        if len(sk) == 1 or len(tk) == 1:
            meant = [(a, b) for a in sk for b in tk]
        else:
            meant = [(a, a) for a in sk if a in st_shapes] or list(zip(sk, tk))
        for a, b in meant:
            if seq_shapes[a].length != st_shapes[b].length:
                fasta.eprint("-p motif %s is %d positions wide and -q motif %s %d: they share no window" %
                             (a, seq_shapes[a].length, b, st_shapes[b].length))
                return None
    elif st_shapes is not None:
        pairs = [(None, b) for b in st_shapes]                     # the file's motif order, as for a structure FASTA
    else:
        pairs = [(a, None) for a in seq_shapes]
    if st_shapes is not None and not _widths_ok(st_shapes, [b for _, b in pairs], "-q", args.pfm_struct):
        return None
    if seq_shapes is not None and not _widths_ok(seq_shapes, [a for a, _ in pairs], "-p", args.pfm_seq):
        return None
    return pairs, st_shapes, seq_shapes


def profile_sources(args, engine):
    """the inputs of an averaged-structure run once a device is open: -> (recs | None, profiles, seq_odds | None,
    struct_odds | None, bg_seq, bg_struct).  With ``-p`` the FASTA's records (ids unique) and the profiles matched to them
    by id in the FASTA's order; the row dtype is ``--profile-dtype``, else the store's own, else float64; the structure
    background is ``-u``, ``-B`` or the profiles' own (background.profile_background).  Shared with ``expect_profile``."""
    from . import background, pssm, sites, store
    source = args.inputs[-1]
    stored = store.ProfileStore(source).dtype if store.is_store(source) else None
    dtype = np.dtype(args.profile_dtype).type if args.profile_dtype else (np.dtype(stored).type if stored is not None else np.float64)
    recs = None
    if args.pfm_seq:
        recs = fasta.open_lazy(args.inputs[0])
        if len(set(recs.ids)) != len(recs):
            seen = set()
            dup = next(i for i in recs.ids if i in seen or seen.add(i))
            raise sites.InputError("record %s occurs more than once in the FASTA" % dup)
        profiles = sites._Profiles(source, dtype, order=list(recs.ids))
    else:
        profiles = sites._Profiles(source, dtype)
    bg_struct = struct_odds = None
    if args.pfm_struct:
        if args.uniform_background:
            bg_struct = None
        elif args.bg_struct:
            bg_struct = fasta.load_background(args.bg_struct, False, source, fasta.STRUCT, True)
        else:
            bg_struct = background.profile_background(engine, source)
        struct_odds = pssm.load_odds(args.pfm_struct, args.pseudocount, fasta.STRUCT, bg_struct)
    bg_seq = seq_odds = None
    if args.pfm_seq:
        bg_seq = fasta.load_background(args.bg_seq, args.uniform_background, args.inputs[0], fasta.RNA, True)
        seq_odds = pssm.load_odds(args.pfm_seq, args.pseudocount, fasta.RNA, bg_seq)
    return recs, profiles, seq_odds, struct_odds, bg_seq, bg_struct


def paired_batch(recs, at, ids, pst):
    """the stream of one run of ``profiles.runs``: the profile's own (structure only, ``recs`` None), or the codes of the
    FASTA's records at..at+len(ids) beside the rows; a record whose length is not its profile's is an InputError"""
    from . import scanner, sites
    if recs is None:
        return pst
    batch = scanner._RnaBatch(recs[at:at + len(ids)])
    if not np.array_equal(batch.lengths, pst.lengths):
        r = int(np.flatnonzero(batch.lengths != pst.lengths)[0])
        raise sites.InputError("record %s is %d letters long but its averaged-structure profile has %d rows" %
                               (ids[r], int(batch.lengths[r]), int(pst.lengths[r])))
    return pack.Stream(batch.codes, pst.profile, batch.offsets, batch.lengths)


def single_fasta(args, dev):
    """the prologue of a run on one FASTA of letters (``occupancy`` and ``expect`` with -p or -q): the motifs and their widths
    before any device work, then the engine, a dot-bracket file annotated, the background, the odds and the records ->
    (motif ids, letters, code letters, background, odds, records) or None (said on stderr)"""
    from . import cli, pssm
    seq = bool(args.pfm_seq)
    option, pfm_file = ("-p", args.pfm_seq) if seq else ("-q", args.pfm_struct)
    letters, code_letters = (fasta.RNA, pack.RNA_LETTERS) if seq else (fasta.STRUCT, pack.STRUCT_LETTERS)
    shapes = _load_shapes(pfm_file, option, args.pseudocount, letters)
    if shapes is None:
        return None
    motif_ids = list(shapes.keys()) if args.all_motifs else [next(iter(shapes))]
    if not _widths_ok(shapes, motif_ids, option, pfm_file):
        return None
    engine = dev.engine
    source = args.fasta
    if not seq:
        # a dot-bracket structure FASTA is annotated first and replaced by its letters (cli.struct_input)
        ns = argparse.Namespace(fastafiles=[args.fasta], struct_format=args.struct_format, testseq=None)
        cli.struct_input(ns, "SS", None, lambda: engine)
        source = ns.fastafiles[0]
    bg = fasta.load_background(args.bg_seq if seq else args.bg_struct, args.uniform_background, source, letters, True)
    odds = pssm.load_odds(pfm_file, args.pseudocount, letters, bg)
    return motif_ids, letters, code_letters, bg, odds, fasta.open_lazy(source)


def main_profiles(args, engine, out):
    """the averaged-structure modes: ``-q st.pfm avgdir_or_store`` and ``-p seq.pfm -q st.pfm seqs.fa avgdir_or_store``"""
    from . import background, sites
    with Device(engine, args.device, (IOError, sites.InputError, background.BackgroundError, background.InputError)) as dev:
        motifs = profile_motifs(args)
        if motifs is None:
            return 1
        pairs = motifs[0]
        engine = dev.engine
        recs, profiles, seq_odds, struct_odds, _, _ = profile_sources(args, engine)
        groups = _by_width([struct_odds[b].length for _, b in pairs])
        tables = profile_tables(seq_odds, struct_odds, pairs, args.pairing)
        write_table(out, [sites.pair_id(a, b) for a, b in pairs], groups, profile_batches(recs, profiles, args.batch_records),
                    lambda stream, m, ks, cols: engine.occupancy_profile(stream, *tables(m, ks, cols)))
        return 0
    return 1


def main(argv=None, engine=None, out=None):
    args = getoptions(argv)
    out = sys.stdout if out is None else out
    if not args.pfm_seq and not args.pfm_struct:
        fasta.eprint("one of -p (sequence PFM) or -q (structure PFM) is required")
        return 1
    profiles = _is_profiles(args.inputs[-1])
    if args.pfm_seq and args.pfm_struct:
        if len(args.inputs) != 2 or not profiles or _is_profiles(args.inputs[0]):
            fasta.eprint("-p with -q needs the sequence FASTA and an averaged-structure directory or packed store (seqs.fa avgdir/): "
                         "the occupancy of two-FASTA pairs is not supported, run -p and -q one at a time")
            return 1
        return main_profiles(args, engine, out)
    if len(args.inputs) == 2:
        fasta.eprint("%s alone takes one input: give -p and -q with the sequence FASTA and the averaged-structure directory or store" %
                     ("-p" if args.pfm_seq else "-q"))
        return 1
    if profiles:
        if args.pfm_seq:
            fasta.eprint("-p alone needs a sequence FASTA, %s is an averaged-structure directory or store: give -q, or -p with -q and both inputs" % args.inputs[0])
            return 1
        return main_profiles(args, engine, out)
    with Device(engine, args.device, (IOError,)) as dev:
        got = single_fasta(args, dev)
        if got is None:
            return 1
        motif_ids, letters, code_letters, _, odds, recs = got
        engine = dev.engine
        groups = _by_width([odds[mid].length for mid in motif_ids])
        tables = dict((m, np.stack([odds[motif_ids[k]].ratio_table(code_letters) for k in ks])) for m, ks in groups.items())
        write_table(out, motif_ids, groups, letter_batches(recs, letters, args.batch_records),
                    lambda stream, m, ks, cols: engine.occupancy(stream, tables[m], len(code_letters)))
        return 0
    return 1


if __name__ == "__main__":
    sys.exit(main())
