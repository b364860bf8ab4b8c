"""Site profiles: what the sites of a motif look like.

``rnascan -p .. -q .. seqs.fa avgdir/`` prints where a motif pair hits; this module answers the next question: the
structural context (and the letters) under those hits, and over ``--flank`` columns either side of them -- the
meta-profile -- summed over all sites and normalised per position.  That is also what a structure PFM is made from: the
reference builds its averaged profiles by counting aligned context letters (average_structure.py:28-42) and normalising
per position (``norm_pfm``, pfmutil.py:136-151); summing the profile rows under aligned hit windows is the same
operation on hits.  With ``--flank 0`` the output is a PFM that ``-p`` / ``-q`` read, which closes the loop
fold -> average -> background -> scan -> site PFM -> scan again.

    column j of a hit at stream position p   row p - F + j of the hit's record, j in [0, W), W = m + 2 F; columns that
                                             hang over a record end are skipped (coverage n[j] counts the others)
    S[j][c]       the sum of profile[row][c] over the hits whose column j counts
    counts[j][k]  the number of those hits whose letter there is k (A, C, G, U; anything else is foreign)
    structure PFM row j = S[j][c] / sum over c of S[j][c]            (norm_pfm: columns BEHLMRT, summed left to right)
    letter PFM    row j = counts[j][letter] / sum over A, C, G, U     (foreign letters excluded, and reported)

The sums are made on the GPU per GROUP of at most 4096 hits of a record (``HipEngine.site_sums``: a fixed order of
additions inside a group, see include/pfmscan.h) and the groups are combined here with ``math.fsum``, which is exactly
rounded: the result has the same bits whatever the batch size, the pipeline chunk, the upload mode, the input form and
the number of ranks.  Profile columns are matched to letters by NAME, file by file for a directory.

``--all-motifs``: one profile per motif (pair) of multi-PFM files from ONE pass per PFM width.  The hits come from the library
kernels, and the group rows are not brought home: the GPU adds them per motif into exact integer accumulators
(``HipEngine.site_sums_library``; 66 limbs of 64 bits per cell, include/pfmscan.h), which are merged over batches and ranks
and rounded once -- per motif the bits of the ``math.fsum`` above.

FASTA inputs (the last input is a file): ``-p seqs.fa``, ``-q structs.fa``, ``-p -q seqs.fa structs.fa`` and ``-p seqs.fa
structs.fa`` (the sequence motif's hits with the structure letters under them).  The structure side is then a letter
string and the site PFM is the reference's own PFM builder on the hit windows: ``struct_pfm_from_aligned`` counts letters
per position (average_structure.py:28-42), ``norm_pfm`` divides each row by its sum (pfmutil.py:136-151).  The GPU counts
letter PAIRS per column (``HipEngine.site_joint``: uint64 [n][W][8][8], include/pfmscan.h); the letter counts of either
stream are the table's marginals, the coverage its column sums, and with two files PREFIX.joint.txt shows which nucleotide
sits in which structural context.  Integers: batches and ranks add, the bytes do not depend on how the input was cut.
"""
import argparse
import math
import os
import sys

import numpy as np

from . import fasta, pack, shard, store

STRUCT_ORDER = pack.STRUCT_COLUMNS         # column order of the structure PFMs this writes (the shipped PFMs': BEHLMRT)
SEQ_ORDER = pack.RNA_LETTERS               # ... and of the sequence PFMs (ACGU); code k of a stream is SEQ_ORDER[k]


class SitesError(ValueError):
    """a cell under a site from which no profile can be computed; ``record``, ``position`` (1-based) and ``letter`` say where"""

    def __init__(self, record, position, letter, value):
        ValueError.__init__(self, "Averaged-structure profile %s holds %r at position %d, column %s, under a site: no site "
                                  "profile can be computed from it (fix the profile)" % (record, value, position, letter))
        self.record, self.position, self.letter, self.value = record, position, letter, value

    def __reduce__(self):            # ranks hand it to each other (combine): rebuilt from its four fields
        return (SitesError, (self.record, self.position, self.letter, self.value))


class InputError(ValueError):
    """inputs no site profile can be read from (the message says which record or file and why)"""


class Rows(object):
    """what one rank collected: group sums float64 [n][W][7] (columns in STRUCT_ORDER) or None, letter counts int64
    [W][8] or None, coverage int64 [W], the number of hits"""

    def __init__(self, W, profile=True, letters=True):
        self.W = W
        self.sums = [] if profile else None
        self.counts = np.zeros((W, 8), dtype=np.int64) if letters else None
        self.coverage = np.zeros(W, dtype=np.int64)
        self.hits = 0

    def packed(self):
        sums = None
        if self.sums is not None:
            sums = np.concatenate(self.sums) if self.sums else np.zeros((0, self.W, 7), dtype=np.float64)
        return sums, self.counts, self.coverage, self.hits


def coverage(stream, pos, m, flank):
    """n[j], int64 [W]: the number of hits whose column j lies inside the hit's record, from positions and record bounds"""
    W = m + 2 * flank
    pos = np.asarray(pos, dtype=np.int64)
    if pos.size == 0:
        return np.zeros(W, dtype=np.int64)
    rec, start = stream.locate(pos)
    # column j counts iff 0 <= start - flank + j < length: per hit a run [lo, hi) of columns
    lo = np.clip(flank - start, 0, W)
    hi = np.clip(stream.lengths[rec] - start + flank, 0, W)
    edge = np.zeros(W + 1, dtype=np.int64)
    np.add.at(edge, lo, 1)
    np.add.at(edge, hi, -1)
    return np.cumsum(edge[:-1])


def accumulate(engine, rows, stream, ids, letters_of, pos, m, flank=0):
    """add the sites ``pos`` (sorted stream positions of windows of width m) of one packed batch to ``rows``.
    ``letters_of(record index in the batch)`` -> that record's profile column letters (for messages);
    the batch's columns are ``letters_of(0)`` and are put into STRUCT_ORDER by name."""
    pos = np.asarray(pos, dtype=np.int64)
    if pos.size == 0:
        return
    try:
        _, sums, counts = engine.site_sums(stream, pos, m, flank, letters=rows.counts is not None, profile=rows.sums is not None)
    except ValueError as e:
        at = getattr(e, "element", None)
        if at is None:
            raise
        row, col = divmod(int(at), 7)
        rec, start = stream.locate(np.asarray([row]))
        rec = int(rec[0])
        raise SitesError(ids[rec], int(start[0]) + 1, letters_of(rec)[col], float(stream.profile[row, col]))
    if rows.sums is not None:
        cols = list(letters_of(0))
        if sorted(cols) != sorted(STRUCT_ORDER):
            raise InputError("averaged-structure columns %s are not the seven structure letters %s" % (cols, STRUCT_ORDER))
        if cols != list(STRUCT_ORDER):
            sums = sums[:, :, [cols.index(c) for c in STRUCT_ORDER]]
        rows.sums.append(np.ascontiguousarray(sums))
    if rows.counts is not None:
        rows.counts += counts.astype(np.int64).sum(axis=0)
    rows.coverage += coverage(stream, pos, m, flank)
    rows.hits += int(pos.size)


def _portable(e):
    """an exception another rank can rebuild"""
    import pickle
    try:
        pickle.loads(pickle.dumps(e))
        return e
    except Exception:
        return RuntimeError("%s: %s" % (type(e).__name__, e))


def combine(rows, rank=0, world=1, dist=None, failure=None):
    """the ranks' rows -> (S float64 [W][7] | None, counts int64 [W][8] | None, coverage int64 [W], hits), the same on
    every rank.  The rows are exchanged once over the process group, host side; a rank that failed hands its exception
    over instead (``failure``), and every rank raises the one of the lowest rank (shares are contiguous and in rank
    order: for a rejected cell that is the earliest in input order).  Then math.fsum per cell over every group."""
    if world > 1:
        shares = [None] * world
        dist.all_gather_object(shares, (None if failure is None else _portable(failure), None if failure is not None else rows.packed()))
        for bad, _ in shares:
            if bad is not None:
                raise bad
        parts = [s for _, s in shares]
    else:
        if failure is not None:
            raise failure
        parts = [rows.packed()]
    W = rows.W
    S = counts = None
    if parts[0][0] is not None:
        groups = np.concatenate([p[0] for p in parts])
        S = np.zeros((W, 7), dtype=np.float64)
        flat = np.ascontiguousarray(groups.reshape(groups.shape[0], W * 7).T)
        for e in range(W * 7):
            S[e // 7, e % 7] = math.fsum(flat[e].tolist())
    if parts[0][1] is not None:
        counts = np.sum([p[1] for p in parts], axis=0, dtype=np.int64)
    cov = np.sum([p[2] for p in parts], axis=0, dtype=np.int64)
    return S, counts, cov, int(sum(p[3] for p in parts))


def site_pfms(S, counts):
    """(structure PFM float64 [W][7] in STRUCT_ORDER | None, letter PFM float64 [W][4] in SEQ_ORDER | None, foreign
    letters int64 [W] | None).  A row without mass is an error that names the column."""
    struct = seq = foreign = None
    if S is not None:
        total = np.zeros(S.shape[0], dtype=np.float64)
        for c in range(7):                         # norm_pfm (pfmutil.py:136-151): 0 + B + E + ... left to right
            total = total + S[:, c]
        empty = np.flatnonzero(~(total > 0))
        if empty.size:
            raise InputError("column %d of the site profile has no structure mass under any site (every site skips it, or "
                             "the profile rows there are zero): it cannot be normalised" % int(empty[0]))
        struct = S / total[:, None]
    if counts is not None:
        known = counts[:, :len(SEQ_ORDER)]
        total = known.sum(axis=1)
        empty = np.flatnonzero(total == 0)
        if empty.size:
            raise InputError("column %d of the site profile has no nucleotide under any site: it cannot be normalised" % int(empty[0]))
        seq = known / total[:, None].astype(np.float64)
        foreign = counts[:, len(SEQ_ORDER):].sum(axis=1)
    return struct, seq, foreign


def write_pfm(path, letters, matrix):
    """the PFM text format ``-p`` / ``-q`` read: header PO + letters, one row per position, every number in the shortest
    form that reads back to the same float64 (the native table writer, pfmscan_tsv_format)"""
    with open(path, "w") as out:
        _pfm_to(out, letters, matrix)


def _pfm_to(out, letters, matrix):
    from . import table
    matrix = np.asarray(matrix)
    w = table.TsvWriter(out, ["PO"] + list(letters), match_id=False)
    cols = {"PO": np.arange(matrix.shape[0], dtype=np.int64)}
    for k, c in enumerate(letters):
        cols[c] = np.ascontiguousarray(matrix[:, k])
    w.write_chunk(cols, matrix.shape[0])
    w.close()


def write_counts(path, S, counts, cov, hits):
    """PREFIX.counts.txt: per column the coverage, the raw structure sums and the integer letter counts (N = foreign)"""
    with open(path, "w") as out:
        _counts_to(out, S, counts, cov, hits)


def _counts_to(out, S, counts, cov, hits):
    from . import table
    names, cols = ["PO", "Sites", "Coverage"], {"PO": np.arange(cov.size, dtype=np.int64), "Sites": np.full(cov.size, hits, dtype=np.int64),
                                                "Coverage": cov}
    if S is not None:
        for k, c in enumerate(STRUCT_ORDER):
            names.append("Sum." + c)
            cols["Sum." + c] = np.ascontiguousarray(S[:, k])
    if counts is not None:
        for k, c in enumerate(SEQ_ORDER):
            names.append("Count." + c)
            cols["Count." + c] = np.ascontiguousarray(counts[:, k])
        names.append("Count.N")
        cols["Count.N"] = counts[:, len(SEQ_ORDER):].sum(axis=1)
    w = table.TsvWriter(out, names, match_id=False)
    w.write_chunk(cols, cov.size)
    w.close()


# ---------------------------------------------------------------------------
# hit selection: exactly rnascan's
# ---------------------------------------------------------------------------
def select(engine, stream, m, letter_table, struct_pssm, minscore, min_seqstruct=None, one_shot=True):
    """the stream positions ``rnascan`` reports for this motif (pair) with the same -m / --min-seqstruct: the same
    engine.hits / hits_sum calls as scanner._scan_combined_stream, scan_records and _scan_profile_stream make"""
    from . import scanner
    thr = float(minscore)
    both = letter_table is not None and struct_pssm is not None
    if both and min_seqstruct is not None and hasattr(engine, "hits_sum"):
        pos, _, _ = engine.hits_sum(stream, letter_table, struct_pssm, thr, thr, float(min_seqstruct), one_shot=one_shot)
        return pos
    pos, sq, st = scanner._select(engine, stream, m, letter_table, struct_pssm, thr if letter_table is not None else -np.inf,
                                  thr if struct_pssm is not None else -np.inf, one_shot=one_shot)
    if both and min_seqstruct is not None:
        keep = np.round(sq, 3).astype(np.float64) + st > float(min_seqstruct)
        pos = pos[keep]
    return pos


def getoptions(argv=None):
    desc = ("Site profiles: the averaged-structure rows (and the nucleotides) under the hits rnascan would report with the same "
            "options, summed over all sites and normalised per position.  Writes PREFIX.struct.txt (structure PFM over "
            "W = width + 2 x flank columns), PREFIX.seq.txt (sequence PFM; only with a FASTA) and PREFIX.counts.txt (raw "
            "sums, integer counts, coverage and number of sites per column).  On FASTA inputs alone the structure side is a "
            "letter string: the letters under the hits are counted instead, and with two files PREFIX.joint.txt holds the "
            "nucleotide x structure letter counts per column.")
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.sites", description=desc)
    parser.add_argument("inputs", metavar="INPUT", nargs="+",
                        help=("seqs.fa avgdir_or_store/ (with -p), or avgdir_or_store/ alone (with -q only); or FASTA inputs as "
                              "rnascan takes them: seqs.fa (-p), structs.fa (-q), seqs.fa structs.fa (-p -q, or -p alone: the "
                              "sequence motif's sites with the structure letters under them), which also write PREFIX.joint.txt "
                              "(nucleotide x structure letter counts per column) when there are two files"))
    parser.add_argument("-p", "--pfm_seq", dest="pfm_seq", type=str, help="Sequence PFM (the first motif of a multi-PFM file; every motif with --all-motifs)")
    parser.add_argument("-q", "--pfm_struct", dest="pfm_struct", type=str, help="Structure PFM (the first motif of a multi-PFM file; every motif with --all-motifs)")
    parser.add_argument("-C", "--pseudocount", type=float, dest="pseudocount", default=0, help="Pseudocount for normalizing PFM. [%(default)s]")
    parser.add_argument("-m", "--minscore", type=float, dest="minscore", default=6, help="Minimum score for motif hits. [%(default)s]")
    parser.add_argument("--min-seqstruct", type=float, default=None, dest="min_seqstruct", metavar="T",
                        help="with -p AND -q: additionally keep a site only if its LogOdds.SeqStruct exceeds T, as rnascan does [off]")
    parser.add_argument("--all-motifs", action="store_true", default=False, dest="all_motifs",
                        help=("one site profile per motif (pair) of multi-PFM files, pairs as rnascan pairs them, in one pass per "
                              "width: PREFIX.struct.txt / PREFIX.seq.txt become multi-PFM libraries that -q / -p read, "
                              "PREFIX.counts.txt gets a leading Motif column [off]"))
    parser.add_argument("--flank", type=int, default=0, metavar="F",
                        help=("also sum F columns either side of every site; columns that hang over a record end are skipped.  "
                              "NOTE: only --flank 0 writes a PFM of the motif's width that -q / -p accept as the motif it came from; "
                              "with F > 0 the files are a profile plot over the flanks, not a PFM for -q [%(default)s]"))
    parser.add_argument("-u", "--uniformbg", action="store_true", default=False, dest="uniform_background",
                        help="Use uniform background for calculating log-odds [%(default)s]")
    parser.add_argument("-b", "--bg_seq", default=None, dest="bg_seq", help="File of pre-computed background probabilities for sequences")
    parser.add_argument("-B", "--bg_struct", default=None, dest="bg_struct", help="File of pre-computed background probabilities for structure")
    parser.add_argument("--pairing", choices=["aligned", "positional"], default="aligned", help="as rnascan's [%(default)s]")
    parser.add_argument("--profile-dtype", choices=["auto", "float64", "float32"], default="float64", help="as rnascan's [%(default)s]")
    parser.add_argument("--struct-format", choices=["auto", "letters", "dotbracket"], default="auto", dest="struct_format",
                        help="a structure FASTA: as rnascan's, without the fragment formats [%(default)s]")
    parser.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")
    parser.add_argument("--gpus", type=int, default=None, help="one process per GPU, records sharded over them, as rnascan's [1]")
    parser.add_argument("-o", "--output", dest="prefix", required=True, metavar="PREFIX", help="prefix of the files written")
    args = parser.parse_args(argv)
    if not (args.pfm_seq or args.pfm_struct):
        parser.error("Must specify PFMs with -p and/or -q")
    if args.uniform_background and (args.bg_seq or args.bg_struct):
        parser.error("You cannot set uniform and custom background options at the same time\n")
    if args.min_seqstruct is not None and not (args.pfm_seq and args.pfm_struct):
        parser.error("--min-seqstruct thresholds the combined score: it needs both -p and -q")
    if args.min_seqstruct is not None and args.min_seqstruct != args.min_seqstruct:
        parser.error("--min-seqstruct: not a number")
    if args.flank < 0:
        parser.error("--flank must be at least 0")
    if args.pfm_seq and args.pfm_struct and len(args.inputs) != 2:
        parser.error("with -p and -q give the sequence FASTA and the averaged-structure directory, store or structure FASTA")
    if args.pfm_seq and (len(args.inputs) > 2 or (len(args.inputs) == 1 and os.path.isdir(args.inputs[0]))):
        parser.error("with -p give the sequence FASTA and the averaged-structure directory or store (or FASTA files alone)")
    if not args.pfm_seq and len(args.inputs) != 1:
        parser.error("with -q alone give the averaged-structure directory or store (or the structure FASTA) only")
    args.fastafiles = list(args.inputs)
    args.testseq, args.bgonly = None, False
    return args


class _Profiles(object):
    """the averaged-structure input (directory or packed store) as records: ids, lengths (weights for a directory), and
    ``runs(a, b)`` -> [(ids, column letters, pack.Stream without codes)] of records [a, b): one run for a store, one per
    stretch of files with the same column order for a directory (columns are matched by name, file by file)"""

    def __init__(self, source, dtype, order=None):
        self.store = store.ProfileStore(source) if store.is_store(source) else None
        self.dtype = dtype
        self.at = None                             # with ``order``: index of the FASTA's record k among the profiles
        if self.store is not None:
            self.ids = list(self.store.ids)
            self.lengths = self.store.lengths
        else:
            files = fasta.list_profiles(source)
            if len(files) == 0:
                raise IOError("No averaged structure files found")
            self.files = files
            self.ids = [sid for sid, _ in files]
            self.lengths = np.asarray([os.path.getsize(path) // 64 + 1 for _, path in files], dtype=np.int64)
        if order is not None:                      # the FASTA's records in the FASTA's order, one profile each
            where = {}
            for i, sid in enumerate(self.ids):
                if sid in where:
                    raise InputError("record %s has more than one averaged-structure profile" % sid)
                where[sid] = i
            missing = [sid for sid in order if sid not in where]
            if missing:
                raise InputError("record %s of the FASTA has no averaged-structure profile" % missing[0])
            if len(where) != len(order):
                extra = sorted(set(where) - set(order))
                raise InputError("averaged-structure profile %s has no record in the FASTA" % extra[0])
            self.at = [where[sid] for sid in order]
            if self.at == list(range(len(order))):
                self.at = None
            else:
                self.ids = list(order)
                self.lengths = self.lengths[self.at]

    def runs(self, a, b):
        if self.store is not None:
            ps = self.store
            if self.at is None:
                st = ps.stream(a, b)
            else:
                st = pack.pack(profiles=[ps.profile[int(ps.offsets[i]):int(ps.offsets[i] + ps.lengths[i])] for i in self.at[a:b]],
                               profile_dtype=ps.dtype)
            prof = st.profile
            if prof.dtype == np.float64 and np.dtype(self.dtype) == np.float32:
                prof = np.asarray(prof, dtype=np.float32)
            return [(self.ids[a:b], list(ps.letters), pack.Stream(None, prof, st.offsets, st.lengths))]
        idx = list(range(a, b)) if self.at is None else self.at[a:b]
        parsed = fasta.read_profiles([self.files[i][1] for i in idx])
        out, k = [], 0
        while k < len(parsed):
            e = k + 1
            while e < len(parsed) and list(parsed[e][0]) == list(parsed[k][0]):
                e += 1
            st = pack.pack(profiles=[p for _, p in parsed[k:e]], profile_dtype=self.dtype)
            out.append((self.ids[a + k:a + e], list(parsed[k][0]), st))
            k = e
        return out


def collect(engine, args, seq_pssm, struct_pssm, rank=0, world=1):
    """this rank's Rows: its share of the records, batch by batch, sites selected as rnascan selects its hits"""
    from . import cli, scanner
    seq_id, seq_pm = scanner._first_motif(seq_pssm) if seq_pssm else (None, None)
    st_id, st_pm = scanner._first_motif(struct_pssm) if struct_pssm else (None, None)
    if seq_pm is not None and st_pm is not None and seq_pm.length != st_pm.length:
        raise InputError("the sequence PFM is %d positions wide and the structure PFM %d: they share no site" % (seq_pm.length, st_pm.length))
    m = (seq_pm or st_pm).length
    W = m + 2 * args.flank
    from ._lib import MAX_WIDTH
    if W > MAX_WIDTH:
        raise InputError("width %d + 2 x flank %d exceeds %d columns (PFMSCAN_MAX_WIDTH, include/pfmscan.h)" % (m, args.flank, MAX_WIDTH))
    source = args.fastafiles[-1]
    stored = store.ProfileStore(source).dtype if store.is_store(source) else None
    ptype = cli.profile_type(args, struct_pssm, stored) if struct_pssm else (np.dtype(args.profile_dtype).type if args.profile_dtype != "auto" else np.float64)
    tab = seq_pm.letter_table(pack.RNA_LETTERS) if seq_pm is not None else None
    rows = Rows(W, profile=True, letters=seq_pm is not None)
    if seq_pm is not None:
        recs = fasta.open_lazy(args.fastafiles[0])
        if len(set(recs.ids)) != len(recs):
            seen = set()
            dup = next(i for i in recs.ids if i in seen or seen.add(i))
            raise InputError("record %s occurs more than once in the FASTA" % dup)
        profiles = _Profiles(source, ptype, order=list(recs.ids))
        lengths = recs.lengths
    else:
        recs = None
        profiles = _Profiles(source, ptype)
        lengths = profiles.lengths
    lo, hi = shard.partition(lengths, world)[rank]
    for a, b in (shard.batches(lengths, lo, hi, shard.batch_positions()) if hi > lo else []):
        at = a
        for ids, cols, pst in profiles.runs(a, b):
            n = len(ids)
            stream = pst
            if recs is not None:
                batch = scanner._RnaBatch(recs[at:at + n])
                if not np.array_equal(batch.lengths, pst.lengths):
                    r = int(np.flatnonzero(batch.lengths != pst.lengths)[0])
                    raise InputError("record %s is %d letters long but its averaged-structure profile has %d rows" %
                                     (ids[r], int(batch.lengths[r]), int(pst.lengths[r])))
                stream = pack.Stream(batch.codes, pst.profile, batch.offsets, batch.lengths)
            P = scanner.struct_matrix(st_pm, cols, args.pairing) if st_pm is not None else None
            pos = select(engine, stream, m, tab, P, args.minscore, args.min_seqstruct)
            accumulate(engine, rows, stream, ids, lambda r, cols=cols: cols, pos, m, args.flank)
            at += n
    return rows, m


def gather(engine, args, seq_pssm, struct_pssm, rank=0, world=1, dist=None):
    """``collect`` on this rank, then ``combine`` over the ranks -> (S, counts, coverage, hits), the same on every rank; a
    rank whose share fails hands its exception over and every rank raises the one of the lowest rank"""
    rows, failure = None, None
    try:
        rows, _ = collect(engine, args, seq_pssm, struct_pssm, rank, world)
    except Exception as e:
        if world == 1:
            raise
        failure = e
        rows = Rows(1)
    return combine(rows, rank, world, dist, failure)


# ---------------------------------------------------------------------------
# --all-motifs: one profile per motif (pair) of multi-PFM files
# ---------------------------------------------------------------------------
ACC_LIMIT = 1 << 31                           # bytes of the long accumulators of one width group


def motif_pairs(seq_pssm, struct_pssm):
    """[(sequence id | None, structure id | None)] in output order: scanner.pair_motifs' pairs, or every motif of the one file"""
    from . import scanner
    if seq_pssm and struct_pssm:
        pairs = scanner.pair_motifs(seq_pssm, struct_pssm)
        if pairs is None:
            raise InputError("the two PFM libraries differ in size and share no motif id: their motifs cannot be paired")
        return pairs
    one = seq_pssm or struct_pssm
    ids = sorted(one.keys()) if len(one) > 1 else list(one.keys())
    return [(i, None) for i in ids] if seq_pssm else [(None, i) for i in ids]


def pair_id(a, b):
    if b is None or a == b:
        return a
    return b if a is None else "%s__%s" % (a, b)


def select_library(engine, stream, m, tabs, pssms, minscore, min_seqstruct=None):
    """(pos, motif index) in (position, motif index) order: for every motif (pair) of one width the positions ``rnascan``
    reports with the same options -- the same library_hits / library_hits_sum / per-pair calls and conditions as
    scanner._scan_combined_stream, scan_records and _scan_profile_stream.  The stream is left staged for the sums."""
    from . import scanner
    thr = float(minscore)
    n = len(tabs if tabs is not None else pssms)
    both = tabs is not None and pssms is not None
    wide = n > 1 and m <= scanner.LIBRARY_MAX_M
    T = None if tabs is None else np.stack(tabs)
    P = None if pssms is None else np.stack(pssms)
    if both:
        on_device = min_seqstruct is not None and hasattr(engine, "hits_sum")
        in_library = on_device and wide and hasattr(engine, "library_hits_sum") and hasattr(engine, "library_sum_thresholds")
        if in_library:
            in_library = bool(np.all(np.isfinite(engine.library_sum_thresholds(stream, T, P, thr, float(min_seqstruct)))))
        if in_library:
            pos, mo, _, _ = engine.library_hits_sum(stream, T, P, thr, thr, float(min_seqstruct))
            return pos, mo
        if not on_device and wide and np.isfinite(thr):
            pos, mo, sq, st = engine.library_hits(stream, T, P, thr, thr, one_shot=False)
            if min_seqstruct is not None:
                keep = np.round(sq, 3).astype(np.float64) + st > float(min_seqstruct)
                pos, mo = pos[keep], mo[keep]
            return pos, mo
    elif wide and np.isfinite(thr) and hasattr(engine, "library_hits"):
        if tabs is not None:
            pos, mo, _, _ = engine.library_hits(stream, T, None, thr, one_shot=False)
        else:
            pos, mo, _, _ = engine.library_hits(stream, None, P, None, thr, one_shot=False)
            rec, start = stream.locate(pos)         # no codes -> no separators: drop windows that run over a record end
            ok = start + m <= stream.lengths[rec]
            pos, mo = pos[ok], mo[ok]
        return pos, mo
    parts = [select(engine, stream, m, None if tabs is None else tabs[k], None if pssms is None else pssms[k], minscore,
                    min_seqstruct, one_shot=False) for k in range(n)]
    pos = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    mo = np.concatenate([np.full(p.size, k, dtype=np.int32) for k, p in enumerate(parts)]) if parts else np.zeros(0, dtype=np.int32)
    order = np.lexsort((mo, pos))
    return pos[order], mo[order]


class LibraryRows(object):
    """what one rank collected for the n motifs of one width: normalised long accumulators uint64 [n][66][W * 7] (cells in
    STRUCT_ORDER) or None, letter counts int64 [n][W][8] or None, coverage int64 [n][W], hits int64 [n]"""

    def __init__(self, n, W, letters=True):
        from ._lib import SITE_LIMBS
        self.acc = np.zeros((n, SITE_LIMBS, W * 7), dtype=np.uint64)
        self.counts = np.zeros((n, W, 8), dtype=np.int64) if letters else None
        self.coverage = np.zeros((n, W), dtype=np.int64)
        self.hits = np.zeros(n, dtype=np.int64)

    def add(self, other):
        from . import _lib
        _lib.site_acc_add(self.acc, other.acc)
        if self.counts is not None:
            self.counts += other.counts
        self.coverage += other.coverage
        self.hits += other.hits


def accumulate_library(engine, rows, stream, ids, cols, pos, mo, m, flank=0):
    """add the sites (pos, motif index) of one packed batch to ``rows``; ``cols``: the batch's profile column letters"""
    from . import _lib
    n, W = rows.hits.size, rows.coverage.shape[1]
    if pos.size == 0:
        return
    try:
        acc, counts = engine.site_sums_library(stream, pos, mo, n, m, flank, letters=rows.counts is not None, profile=True)
    except ValueError as e:
        at = getattr(e, "element", None)
        if at is None:
            raise
        row, col = divmod(int(at), 7)
        rec, start = stream.locate(np.asarray([row]))
        rec = int(rec[0])
        raise SitesError(ids[rec], int(start[0]) + 1, cols[col], float(stream.profile[row, col]))
    cols = list(cols)
    if sorted(cols) != sorted(STRUCT_ORDER):
        raise InputError("averaged-structure columns %s are not the seven structure letters %s" % (cols, STRUCT_ORDER))
    if cols != list(STRUCT_ORDER):
        acc = acc.reshape(n, acc.shape[1], W, 7)[..., [cols.index(c) for c in STRUCT_ORDER]].reshape(n, acc.shape[1], W * 7)
    _lib.site_acc_add(rows.acc, np.ascontiguousarray(acc))
    if rows.counts is not None:
        rows.counts += counts.astype(np.int64)
    for k in range(n):
        mine = pos[mo == k]
        rows.coverage[k] += coverage(stream, mine, m, flank)
        rows.hits[k] += mine.size


def collect_library(engine, args, seq_pssm, struct_pssm, rank=0, world=1):
    """this rank's {width: LibraryRows} and the pairs of every width [(width, [pair])], in pair order"""
    from . import cli, scanner
    from ._lib import MAX_WIDTH, SITE_LIMBS
    by_width = {}
    for a, b in motif_pairs(seq_pssm, struct_pssm):
        by_width.setdefault((seq_pssm[a] if a is not None else struct_pssm[b]).length, []).append((a, b))
    if not by_width:
        raise InputError("no sequence PFM is as wide as the structure PFM it is paired with: they share no site")
    for m, group in by_width.items():
        W = m + 2 * args.flank
        if W > MAX_WIDTH:
            raise InputError("width %d + 2 x flank %d exceeds %d columns (PFMSCAN_MAX_WIDTH, include/pfmscan.h)" % (m, args.flank, MAX_WIDTH))
        if len(group) * W * 7 * SITE_LIMBS * 8 > ACC_LIMIT:
            raise InputError("the %d motifs of width %d need %d bytes of accumulators at --flank %d, more than %d: lower --flank or "
                             "split the library" % (len(group), m, len(group) * W * 7 * SITE_LIMBS * 8, args.flank, ACC_LIMIT))
    source = args.fastafiles[-1]
    stored = store.ProfileStore(source).dtype if store.is_store(source) else None
    ptype = cli.profile_type(args, struct_pssm, stored) if struct_pssm else (np.dtype(args.profile_dtype).type if args.profile_dtype != "auto" else np.float64)
    rows = dict((m, LibraryRows(len(group), m + 2 * args.flank, letters=seq_pssm is not None)) for m, group in by_width.items())
    if seq_pssm is not None:
        recs = fasta.open_lazy(args.fastafiles[0])
        if len(set(recs.ids)) != len(recs):
            seen = set()
            dup = next(i for i in recs.ids if i in seen or seen.add(i))
            raise InputError("record %s occurs more than once in the FASTA" % dup)
        profiles = _Profiles(source, ptype, order=list(recs.ids))
        lengths = recs.lengths
    else:
        recs = None
        profiles = _Profiles(source, ptype)
        lengths = profiles.lengths
    lo, hi = shard.partition(lengths, world)[rank]
    for a, b in (shard.batches(lengths, lo, hi, shard.batch_positions()) if hi > lo else []):
        at = a
        for ids, cols, pst in profiles.runs(a, b):
            n = len(ids)
            stream = pst
            if recs is not None:
                batch = scanner._RnaBatch(recs[at:at + n])
                if not np.array_equal(batch.lengths, pst.lengths):
                    r = int(np.flatnonzero(batch.lengths != pst.lengths)[0])
                    raise InputError("record %s is %d letters long but its averaged-structure profile has %d rows" %
                                     (ids[r], int(batch.lengths[r]), int(pst.lengths[r])))
                stream = pack.Stream(batch.codes, pst.profile, batch.offsets, batch.lengths)
            for m, group in by_width.items():
                tabs = [seq_pssm[x].letter_table(pack.RNA_LETTERS) for x, _ in group] if seq_pssm else None
                pssms = [scanner.struct_matrix(struct_pssm[y], cols, args.pairing) for _, y in group] if struct_pssm else None
                pos, mo = select_library(engine, stream, m, tabs, pssms, args.minscore, args.min_seqstruct)
                accumulate_library(engine, rows[m], stream, ids, cols, pos, mo, m, args.flank)
            at += n
    return rows, list(by_width.items())


def gather_library(engine, args, seq_pssm, struct_pssm, rank=0, world=1, dist=None):
    """``collect_library`` on this rank, the ranks' accumulators exchanged once and added (integer sums: any order gives
    the same limbs), rounded once -> [(pair, S float64 [W][7], counts | None, coverage, hits)] in pair order, the same on
    every rank; failures are handed over as in ``combine``"""
    from . import _lib
    rows, groups, failure = None, None, None
    try:
        rows, groups = collect_library(engine, args, seq_pssm, struct_pssm, rank, world)
    except Exception as e:
        if world == 1:
            raise
        failure = e
    if world > 1:
        shares = [None] * world
        dist.all_gather_object(shares, (None if failure is None else _portable(failure), rows))
        for bad, _ in shares:
            if bad is not None:
                raise bad
        rows = shares[0][1]
        for _, other in shares[1:]:
            for m in rows:
                rows[m].add(other[m])
    out = []
    for m, group in groups:
        r = rows[m]
        W = r.coverage.shape[1]
        S = _lib.site_acc_round(r.acc).reshape(len(group), W, 7)
        for k, pair in enumerate(group):
            out.append((pair, S[k], None if r.counts is None else r.counts[k], r.coverage[k], int(r.hits[k])))
    order = dict((pair, i) for i, pair in enumerate(motif_pairs(seq_pssm, struct_pssm)))
    out.sort(key=lambda x: order[x[0]])
    return out


def write_library(args, results, rank=0):
    """the three files of --all-motifs; a motif without a site or with a column that cannot be normalised is named on
    stderr and left out of the PFM files.  -> exit code"""
    import io
    struct_txt, seq_txt, counts_txt = io.StringIO(), io.StringIO(), io.StringIO()
    written, have_seq = 0, False
    for (a, b), S, counts, cov, hits in results:
        name = pair_id(a, b)
        one = io.StringIO()
        _counts_to(one, S, counts, cov, hits)
        lines = one.getvalue().splitlines(True)
        if not counts_txt.tell():
            counts_txt.write("Motif\t" + lines[0])
        for ln in lines[1:]:
            counts_txt.write(name + "\t" + ln)
        if hits == 0:
            fasta.eprint("Motif %s: no site passes the thresholds, left out" % name)
            continue
        try:
            struct, seq, foreign = site_pfms(S, counts)
        except InputError as e:
            fasta.eprint("Motif %s: %s, left out" % (name, e))
            continue
        if foreign is not None and int(foreign.sum()):
            fasta.eprint("Motif %s: foreign letters under the sites, left out of the sequence PFM: %d (per column: %s)" %
                         (name, int(foreign.sum()), " ".join(str(int(x)) for x in foreign)))
        struct_txt.write("#%s\n#" % name)
        _pfm_to(struct_txt, STRUCT_ORDER, struct)
        struct_txt.write("\n")
        if seq is not None:
            have_seq = True
            seq_txt.write("#%s\n#" % name)
            _pfm_to(seq_txt, SEQ_ORDER, seq)
            seq_txt.write("\n")
        written += 1
    fasta.eprint("Wrote the site profiles of %d of %d motifs" % (written, len(results)))
    if written == 0:
        fasta.eprint("No motif has a site profile: no files written")
        return 1
    if rank == 0:
        for suffix, text in ((".struct.txt", struct_txt), (".seq.txt", seq_txt if have_seq else None), (".counts.txt", counts_txt)):
            if text is not None:
                with open(args.prefix + suffix, "w") as out:
                    out.write(text.getvalue())
    return 0


# ---------------------------------------------------------------------------
# FASTA inputs: the structure side is a letter string; letter and letter-pair counts
# ---------------------------------------------------------------------------
STRUCT_CODES = [pack.STRUCT_LETTERS.index(c) for c in STRUCT_ORDER]      # code of a structure stream per column of STRUCT_ORDER
JOINT_NAMES = ["%s.%s" % (a, b) for a in SEQ_ORDER for b in STRUCT_ORDER]  # the 28 known cells: nucleotide major


def select_letters(engine, stream, m, seq_tabs, struct_tabs, minscore, min_seqstruct=None):
    """(pos, motif index) in (position, motif index) order: for every motif (pair) of one width the positions ``rnascan``
    reports on FASTA inputs with the same options -- the same engine calls under the same conditions as
    scanner.scan_records (one kind of table: ``seq_tabs`` over the nucleotides of ``stream.codes``, or ``struct_tabs`` over
    the structure letters of ``stream.codes``) and scanner.scan_pair (both: nucleotides in ``stream.codes``, structure
    letters in ``stream.codes2``).  The stream is left staged for the counts wherever the call allows it."""
    from . import _lib, scanner
    thr = float(minscore)
    n = len(seq_tabs if seq_tabs is not None else struct_tabs)
    finite = bool(np.isfinite(thr))
    if struct_tabs is None:                                    # scan_records, nucleotides
        if n > 1 and finite and m <= scanner.LIBRARY_MAX_M:
            pos, mo, _, _ = engine.library_hits(stream, np.stack(seq_tabs), None, thr, one_shot=False)
            return pos, mo
        parts = [scanner._select(engine, stream, m, t, None, thr, -np.inf, one_shot=False)[0] for t in seq_tabs]
    elif seq_tabs is None:                                     # scan_records, a generic alphabet: fp64 scores
        if n > 1 and finite and m <= scanner.LETTER_LIBRARY_MAX_M and hasattr(engine, "library_hits_letters"):
            pos, mo, _, _ = engine.library_hits_letters(stream, None, np.stack(struct_tabs), None, thr)
            return pos, mo
        parts = [scanner._select_letters_f64(engine, stream, m, t, thr)[0] for t in struct_tabs]
    else:                                                      # scan_pair
        on_device = min_seqstruct is not None and hasattr(engine, "hits_pair_sum") and not np.isnan(float(min_seqstruct))

        def kept(pos, mo, sq, st):                             # scan_pair's rows(): keep_seqstruct on the PRINTED sum
            if min_seqstruct is not None:
                keep = np.round(sq, 3).astype(np.float64) + _lib.round_decimals(st, 3) > float(min_seqstruct)
                pos, mo = pos[keep], (None if mo is None else mo[keep])
            return pos, mo

        if on_device and n > 1 and m <= scanner.LIBRARY_MAX_M and hasattr(engine, "library_hits_letters_sum") and \
                hasattr(engine, "library_letters_sum_thresholds"):
            T, S = np.stack(seq_tabs), np.stack(struct_tabs)
            if np.all(np.isfinite(engine.library_letters_sum_thresholds(T, S, thr, float(min_seqstruct)))):
                return kept(*engine.library_hits_letters_sum(stream, T, S, thr, thr, float(min_seqstruct)))
        elif n > 1 and finite and m <= scanner.LIBRARY_MAX_M and hasattr(engine, "library_hits_letters"):
            return kept(*engine.library_hits_letters(stream, np.stack(seq_tabs), np.stack(struct_tabs), thr, thr))
        parts = []
        for tab_seq, tab_st in zip(seq_tabs, struct_tabs):
            if on_device:
                pos, sq, st = engine.hits_pair_sum(stream, tab_seq, tab_st, thr, thr, float(min_seqstruct))
            elif np.isneginf(thr) or not hasattr(engine, "hits_pair"):
                sq, _ = engine.scan(stream, tab_seq, None)
                st = engine.scan_letters_f64(pack.Stream(stream.codes2, None, stream.offsets, stream.lengths), tab_st)
                pos = np.flatnonzero(stream.window_mask(m) & (sq.astype(np.float64) > thr) & (st > thr))
                sq, st = sq[pos], st[pos]
            else:
                pos, sq, st = engine.hits_pair(stream, tab_seq, tab_st, thr, thr)
            parts.append(kept(pos, None, sq, st)[0])
    pos = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    mo = np.concatenate([np.full(p.size, k, dtype=np.int32) for k, p in enumerate(parts)]) if parts else np.zeros(0, dtype=np.int32)
    order = np.lexsort((mo, pos))
    return pos[order], mo[order]


class LetterRows(object):
    """what one rank collected on FASTA inputs for the n motifs (pairs) of one width: joint int64 [n][W][8][8] -- cell
    [a][b]: nucleotide code a (SEQ_ORDER, 7 foreign), structure code b (pack.STRUCT_LETTERS, 7 foreign); the index of a
    stream that is absent is 0 -- and hits int64 [n]"""

    def __init__(self, n, W):
        self.joint = np.zeros((n, W, 8, 8), dtype=np.int64)
        self.hits = np.zeros(n, dtype=np.int64)

    def add(self, other):
        self.joint += other.joint
        self.hits += other.hits


def paired_fastas(seq_fasta, struct_fasta):
    """(LazyFasta of the sequences, LazyFasta of the structure strings) of two files that hold the same ids in the same
    order, each once, with equal lengths; anything else is an InputError that names the first offending record (the
    counts need both letters of every position: there is no join fallback here)"""
    recs, srecs = fasta.open_lazy(seq_fasta), fasta.open_lazy(struct_fasta)
    ids, sids = list(recs.ids), list(srecs.ids)
    seen = set()
    for k, sid in enumerate(ids):
        if sid in seen:
            raise InputError("record %s occurs more than once in %s" % (sid, seq_fasta))
        seen.add(sid)
        if k >= len(sids):
            raise InputError("record %s of %s has no record in %s" % (sid, seq_fasta, struct_fasta))
        if sids[k] != sid:
            raise InputError("record %s of %s is paired by position with record %s of %s: the two files must hold the same ids "
                             "in the same order" % (sid, seq_fasta, sids[k], struct_fasta))
    if len(sids) > len(ids):
        raise InputError("record %s of %s has no record in %s" % (sids[len(ids)], struct_fasta, seq_fasta))
    a, b = np.asarray(recs.lengths, dtype=np.int64), np.asarray(srecs.lengths, dtype=np.int64)
    if not np.array_equal(a, b):
        r = int(np.flatnonzero(a != b)[0])
        raise InputError("record %s is %d letters long but its structure string has %d" % (ids[r], int(a[r]), int(b[r])))
    return recs, srecs


def collect_letters(engine, args, seq_pssm, struct_pssm, rank=0, world=1):
    """this rank's {width: LetterRows} and the pairs of every width [(width, [pair])]: its share of the records, batch by
    batch, sites selected as rnascan selects its hits (select_letters), counted by ``engine.site_joint``"""
    from . import scanner
    from ._lib import MAX_WIDTH
    two = len(args.fastafiles) == 2
    if args.all_motifs:
        pairs = motif_pairs(seq_pssm, struct_pssm)
    else:
        a = scanner._first_motif(seq_pssm)[0] if seq_pssm else None
        b = scanner._first_motif(struct_pssm)[0] if struct_pssm else None
        if a is not None and b is not None and seq_pssm[a].length != struct_pssm[b].length:
            raise InputError("the sequence PFM is %d positions wide and the structure PFM %d: they share no site" %
                             (seq_pssm[a].length, struct_pssm[b].length))
        pairs = [(a, b)]
    by_width = {}
    for a, b in pairs:
        by_width.setdefault((seq_pssm[a] if a is not None else struct_pssm[b]).length, []).append((a, b))
    if not by_width:
        raise InputError("no sequence PFM is as wide as the structure PFM it is paired with: they share no site")
    for m, group in by_width.items():
        W = m + 2 * args.flank
        if W > MAX_WIDTH:
            raise InputError("width %d + 2 x flank %d exceeds %d columns (PFMSCAN_MAX_WIDTH, include/pfmscan.h)" % (m, args.flank, MAX_WIDTH))
        if len(group) * W * 64 * 8 > ACC_LIMIT:
            raise InputError("the %d motifs of width %d need %d bytes of letter-pair counts at --flank %d, more than %d: lower --flank "
                             "or split the library" % (len(group), m, len(group) * W * 64 * 8, args.flank, ACC_LIMIT))
    rows = dict((m, LetterRows(len(group), m + 2 * args.flank)) for m, group in by_width.items())
    if two:
        recs, srecs = paired_fastas(args.fastafiles[0], args.fastafiles[1])
    else:
        recs, srecs = fasta.open_lazy(args.fastafiles[0]), None
    lengths = recs.lengths
    lo, hi = shard.partition(lengths, world)[rank]
    for a, b in (shard.batches(lengths, lo, hi, shard.batch_positions()) if hi > lo else []):
        if two:
            sb, tb = scanner._RnaBatch(recs[a:b]), scanner._RnaBatch(srecs[a:b], fasta.STRUCT)
            if not np.array_equal(sb.lengths, tb.lengths):
                r = int(np.flatnonzero(sb.lengths != tb.lengths)[0])
                raise InputError("record %s is %d letters long but its structure string has %d" %
                                 (sb.ids[r], int(sb.lengths[r]), int(tb.lengths[r])))
            stream = pack.Stream(sb.codes, None, sb.offsets, sb.lengths, codes2=tb.codes)
        else:
            sb = scanner._RnaBatch(recs[a:b], None if seq_pssm else fasta.STRUCT)
            stream = pack.Stream(sb.codes, None, sb.offsets, sb.lengths)
        for m, group in by_width.items():
            tabs = [seq_pssm[x].letter_table(pack.RNA_LETTERS) for x, _ in group] if seq_pssm else None
            stabs = [struct_pssm[y].letter_table(fasta.STRUCT) for _, y in group] if struct_pssm else None
            pos, mo = select_letters(engine, stream, m, tabs, stabs, args.minscore, args.min_seqstruct)
            if pos.size == 0:
                continue
            n = len(group)
            J = engine.site_joint(stream, pos, None if n == 1 else mo, n, m, args.flank, first=True, second=two).astype(np.int64)
            if not two and not seq_pssm:                       # the one stream holds the structure letters
                J = J.transpose(0, 1, 3, 2)
            rows[m].joint += J
            rows[m].hits += np.bincount(mo, minlength=n).astype(np.int64)
    return rows, list(by_width.items())


def gather_letters(engine, args, seq_pssm, struct_pssm, rank=0, world=1, dist=None):
    """``collect_letters`` on this rank, the ranks' integer tables exchanged once and added -> [(pair, joint int64
    [W][8][8], hits)] in pair order, the same on every rank; failures are handed over as in ``combine``"""
    rows, groups, failure = None, None, None
    try:
        rows, groups = collect_letters(engine, args, seq_pssm, struct_pssm, rank, world)
    except Exception as e:
        if world == 1:
            raise
        failure = e
    if world > 1:
        shares = [None] * world
        dist.all_gather_object(shares, (None if failure is None else _portable(failure), rows))
        for bad, _ in shares:
            if bad is not None:
                raise bad
        rows = shares[0][1]
        for _, other in shares[1:]:
            for m in rows:
                rows[m].add(other[m])
    out = []
    for m, group in groups:
        for k, pair in enumerate(group):
            out.append((pair, rows[m].joint[k], int(rows[m].hits[k])))
    if args.all_motifs:
        order = dict((pair, i) for i, pair in enumerate(motif_pairs(seq_pssm, struct_pssm)))
        out.sort(key=lambda x: order[x[0]])
    return out


def letter_tables(J, has_seq, has_struct):
    """joint int64 [W][8][8] -> (S float64 [W][7] in STRUCT_ORDER | None: the structure letter counts, as float64 for
    ``site_pfms``; nucleotide counts int64 [W][8] | None; structure counts int64 [W][8] by code | None; coverage int64 [W])"""
    seq_counts = J.sum(axis=2) if has_seq else None
    struct_counts = J.sum(axis=1) if has_struct else None
    S = struct_counts[:, STRUCT_CODES].astype(np.float64) if has_struct else None
    return S, seq_counts, struct_counts, J.sum(axis=(1, 2))


def mutual_information(cells):
    """the mutual information, in bits, of a column's 4 x 7 table of known cells (Python ints): math.fsum of
    p_ab log2(p_ab / (p_a p_b)) over the non-zero cells, p = counts / their total; 0.0 for an empty column"""
    total = sum(sum(row) for row in cells)
    if total == 0:
        return 0.0
    pa = [sum(row) / total for row in cells]
    pb = [sum(row[b] for row in cells) / total for b in range(len(cells[0]))]
    return math.fsum((c / total) * math.log2((c / total) / (pa[a] * pb[b]))
                     for a, row in enumerate(cells) for b, c in enumerate(row) if c)


def _letter_counts_to(out, seq_counts, struct_counts, cov, hits):
    """PREFIX.counts.txt on FASTA inputs: coverage and the integer letter counts of the streams present (N / X = foreign)"""
    from . import table
    names = ["PO", "Sites", "Coverage"]
    cols = {"PO": np.arange(cov.size, dtype=np.int64), "Sites": np.full(cov.size, hits, dtype=np.int64), "Coverage": np.ascontiguousarray(cov)}
    if seq_counts is not None:
        for k, c in enumerate(SEQ_ORDER):
            names.append("Count." + c)
            cols["Count." + c] = np.ascontiguousarray(seq_counts[:, k])
        names.append("Count.N")
        cols["Count.N"] = seq_counts[:, len(SEQ_ORDER):].sum(axis=1)
    if struct_counts is not None:
        for k, c in zip(STRUCT_CODES, STRUCT_ORDER):
            names.append("Count." + c)
            cols["Count." + c] = np.ascontiguousarray(struct_counts[:, k])
        names.append("Count.X")
        cols["Count.X"] = np.ascontiguousarray(struct_counts[:, 7])
    w = table.TsvWriter(out, names, match_id=False)
    w.write_chunk(cols, cov.size)
    w.close()


def _joint_to(out, J, mi=mutual_information):
    """PREFIX.joint.txt: per column the 28 known cells A.B A.E ... U.T (nucleotide major, STRUCT_ORDER minor) and MI.  J is
    [W][>= 4][>= 7] by code, counts or (``expect_pair --joint``) expected counts, ``mi`` its mutual information"""
    from . import table
    known = J[:, :len(SEQ_ORDER)][:, :, STRUCT_CODES]
    cols = {"PO": np.arange(J.shape[0], dtype=np.int64)}
    for i, name in enumerate(JOINT_NAMES):
        cols[name] = np.ascontiguousarray(known[:, i // len(STRUCT_ORDER), i % len(STRUCT_ORDER)])
    cols["MI"] = np.asarray([mi(known[j].tolist()) for j in range(J.shape[0])], dtype=np.float64)
    w = table.TsvWriter(out, ["PO"] + JOINT_NAMES + ["MI"], match_id=False)
    w.write_chunk(cols, J.shape[0])
    w.close()


def _report_foreign(prefix, seq_counts, struct_counts):
    for counts, first, what, pfm in ((seq_counts, len(SEQ_ORDER), "letters", "sequence"), (struct_counts, 7, "structure characters", "structure")):
        if counts is None:
            continue
        foreign = counts[:, first:].sum(axis=1)
        if int(foreign.sum()):
            msg = "foreign %s under the sites, left out of the %s PFM: %d (per column: %s)" % \
                (what, pfm, int(foreign.sum()), " ".join(str(int(x)) for x in foreign))
            fasta.eprint(prefix + msg if prefix else msg[0].upper() + msg[1:])


def tagged(text, name, one):
    """the table in ``one`` appended to ``text`` under a leading Motif column: the files that hold one block per motif"""
    lines = one.getvalue().splitlines(True)
    if not text.tell():
        text.write("Motif\t" + lines[0])
    for ln in lines[1:]:
        text.write(name + "\t" + ln)


def write_letters(args, results, has_seq, has_struct, rank=0):
    """the files of the FASTA route (.struct.txt / .seq.txt for the streams present, .joint.txt with both, .counts.txt).
    With --all-motifs a motif without a site or with a column that cannot be normalised is named on stderr and left out
    of the PFM files, as ``write_library`` does; for one motif either is the run's failure.  -> exit code"""
    import io
    if not args.all_motifs:
        _, J, hits = results[0]
        fasta.eprint("Found %d sites" % hits)
        if hits == 0:
            fasta.eprint("No site passes the thresholds: nothing to profile, no files written")
            return 1
        S, seq_counts, struct_counts, cov = letter_tables(J, has_seq, has_struct)
        struct, seq, _ = site_pfms(S, seq_counts)
        _report_foreign("", seq_counts, struct_counts)
        if rank == 0:
            if struct is not None:
                write_pfm(args.prefix + ".struct.txt", STRUCT_ORDER, struct)
            if seq is not None:
                write_pfm(args.prefix + ".seq.txt", SEQ_ORDER, seq)
            if has_seq and has_struct:
                with open(args.prefix + ".joint.txt", "w") as out:
                    _joint_to(out, J)
            with open(args.prefix + ".counts.txt", "w") as out:
                _letter_counts_to(out, seq_counts, struct_counts, cov, hits)
        return 0
    texts = dict((suffix, io.StringIO()) for suffix in (".struct.txt", ".seq.txt", ".joint.txt", ".counts.txt"))
    written = 0

    for (a, b), J, hits in results:
        name = pair_id(a, b)
        S, seq_counts, struct_counts, cov = letter_tables(J, has_seq, has_struct)
        one = io.StringIO()
        _letter_counts_to(one, seq_counts, struct_counts, cov, hits)
        tagged(texts[".counts.txt"], name, one)
        if has_seq and has_struct:
            one = io.StringIO()
            _joint_to(one, J)
            tagged(texts[".joint.txt"], name, one)
        if hits == 0:
            fasta.eprint("Motif %s: no site passes the thresholds, left out" % name)
            continue
        try:
            struct, seq, _ = site_pfms(S, seq_counts)
        except InputError as e:
            fasta.eprint("Motif %s: %s, left out" % (name, e))
            continue
        _report_foreign("Motif %s: " % name, seq_counts, struct_counts)
        for suffix, letters, matrix in ((".struct.txt", STRUCT_ORDER, struct), (".seq.txt", SEQ_ORDER, seq)):
            if matrix is not None:
                texts[suffix].write("#%s\n#" % name)
                _pfm_to(texts[suffix], letters, matrix)
                texts[suffix].write("\n")
        written += 1
    fasta.eprint("Wrote the site profiles of %d of %d motifs" % (written, len(results)))
    if written == 0:
        fasta.eprint("No motif has a site profile: no files written")
        return 1
    if rank == 0:
        for suffix, text in texts.items():
            if text.tell():
                with open(args.prefix + suffix, "w") as out:
                    out.write(text.getvalue())
    return 0


def main_letters(engine, args, rank=0, world=1, dist=None):
    """the FASTA route of ``main``: inputs and backgrounds as cli.main takes them for the same command line"""
    from . import cli
    two = len(args.fastafiles) == 2
    if two and (not os.path.isfile(args.fastafiles[0]) or not args.pfm_seq):
        raise InputError("with two FASTA files give the sequence FASTA first and its PFM with -p (a structure PFM with -q is optional)")
    # a dot-bracket structure FASTA is annotated first and replaced by its letters (cli.struct_input)
    cli.struct_input(args, "RNASS" if two else ("RNA" if args.pfm_seq else "SS"), None, lambda: engine)
    seq_pssm = struct_pssm = None
    if args.pfm_seq:
        bg = fasta.load_background(args.bg_seq, args.uniform_background, args.fastafiles[0], fasta.RNA, True)
        seq_pssm = cli.load_motif(args.pfm_seq, args.pseudocount, fasta.RNA, bg)
    if args.pfm_struct:
        bg = fasta.load_background(args.bg_struct, args.uniform_background, args.fastafiles[-1], fasta.STRUCT, True)
        struct_pssm = cli.load_motif(args.pfm_struct, args.pseudocount, fasta.STRUCT, bg)
    results = gather_letters(engine, args, seq_pssm, struct_pssm, rank, world, dist)
    return write_letters(args, results, has_seq=bool(args.pfm_seq), has_struct=two or not args.pfm_seq, rank=rank)


def main(argv=None, engine=None):
    from . import background, cli, scanner
    args = getoptions(argv)
    if engine is None:
        from . import launch
        world, must_spawn = launch.resolve_world(args.gpus)
        if must_spawn:
            pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            path = os.pathsep.join([pkg_parent] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p])
            rc, _ = launch.spawn_ranks(world, [sys.executable, "-m", "rnascan_amd.sites"] + list(sys.argv[1:] if argv is None else argv),
                                       extra_env={"PYTHONPATH": path})
            return rc
    own = engine is None
    rank, world, dist = cli._init_distributed(args)
    if engine is None:
        engine = scanner.HipEngine(args.device)
    try:
        seq_pssm = struct_pssm = None
        source = args.fastafiles[-1]
        if os.path.isfile(source):                 # FASTA inputs: letter strings (a directory takes the route below)
            rc = main_letters(engine, args, rank, world, dist)
            if dist is not None:
                dist.barrier()
            return rc
        if not os.path.isdir(source):
            raise InputError("%s is neither a directory of structure.<id>.txt files nor a packed profile store" % source)
        if args.pfm_seq:
            bg = fasta.load_background(args.bg_seq, args.uniform_background, args.fastafiles[0], fasta.RNA, True)
            seq_pssm = cli.load_motif(args.pfm_seq, args.pseudocount, fasta.RNA, bg)
        if args.pfm_struct:
            if not args.bg_struct and not args.uniform_background:
                bg = background.profile_background(engine, source, rank, world, dist, True)
            else:
                bg = fasta.load_background(args.bg_struct, args.uniform_background, source, fasta.STRUCT, True)
            struct_pssm = cli.load_motif(args.pfm_struct, args.pseudocount, fasta.STRUCT, bg)
        if args.all_motifs:
            rc = write_library(args, gather_library(engine, args, seq_pssm, struct_pssm, rank, world, dist), rank)
            if dist is not None:
                dist.barrier()
            return rc
        S, counts, cov, hits = gather(engine, args, seq_pssm, struct_pssm, rank, world, dist)
        fasta.eprint("Found %d sites" % hits)
        if hits == 0:
            fasta.eprint("No site passes the thresholds: nothing to profile, no files written")
            return 1
        struct, seq, foreign = site_pfms(S, counts)
        if foreign is not None and int(foreign.sum()):
            fasta.eprint("Foreign letters under the sites, left out of the sequence PFM: %d (per column: %s)" %
                         (int(foreign.sum()), " ".join(str(int(x)) for x in foreign)))
        if rank == 0:
            write_pfm(args.prefix + ".struct.txt", STRUCT_ORDER, struct)
            if seq is not None:
                write_pfm(args.prefix + ".seq.txt", SEQ_ORDER, seq)
            write_counts(args.prefix + ".counts.txt", S, counts, cov, hits)
        if dist is not None:
            dist.barrier()
        return 0
    except (SitesError, InputError, background.BackgroundError, background.InputError) as e:
        if rank == 0:
            fasta.eprint(str(e))
        return 1
    finally:
        if own:
            engine.close()


if __name__ == "__main__":
    sys.exit(main())
