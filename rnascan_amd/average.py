"""Averaged-structure profiles from fragment structures, averaged on the GPU.

Replaces the averaging half of the reference's scripts/run_folding + rnascan/average_structure.py: every record longer
than 50 nt is cut into overlapping windows, each window is folded (RNAfold -p, centroid structure) and annotated to
EHTBLRM, the annotated windows are aligned, counted per position and normalised into ``structure.<id>.txt``
(pfmutil.py:61-87, :136-151).  Folding stays outside; everything around it is here:

  - ``python -m rnascan_amd.average fragments SEQS.fa > frags.fa``: the windows the reference feeds RNAfold, one
    ``>id_frag_i`` record per window (run_folding:63-65, average_structure.py:47-59), without a Python loop per window;
  - ``python -m rnascan_amd.average build FRAGS OUT``: the fragments' structures -- a FASTA of dot-bracket strings named
    ``<id>_frag_<i>``, or RNAfold ``-p`` output (``--input rnafold``) -- averaged into a packed profile store (store.py)
    or a directory of ``structure.<id>.txt`` files byte-identical to write_pfm's.

The annotation and the counting run on the device (pfmscan_average_host: csrc/pfmscan_dotbracket.hip, then
csrc/pfmscan_average.hip).  A row's value in column k is ``T[n(n+1)/2 + c]`` for the row's coverage n and count c:
for a store, what a scan reads back from the reference's text -- pandas' parse of ``str(c / n)`` (``value_table``) --
and for text, ``c / n`` itself, formatted with the shortest repr.  So scanning the text directory, scanning the store
and scanning the fragments (``rnascan --struct-format fragments``) all score the same numbers.

Deviations from the reference: values are written with Python 3's ``str`` (the shortest repr; run_folding is Python 2,
whose ``str`` keeps 12 significant digits); a position no fragment covers is an error naming the record and the
position (the reference raises ZeroDivisionError in norm_pfm); a fragment without any '.' is annotated (all L / R)
where parse_secondary_structure skips the line.
"""
import argparse
import functools
import mmap
import os
import sys
import time

import numpy as np

from . import dotbracket, fasta, store

WINDOW, OVERLAP, MIN_LENGTH = 100, 95, 51          # run_folding's defaults; records of 50 nt or less are skipped (:63-65)
COLUMNS = list("BEHLMRT")                          # write_pfm's column order (sorted letters, pfmutil.py:62)
BATCH_LETTERS = 1 << 27                            # fragment letters averaged per device call (scratch ~ 2 bytes each + rows)
HEADER = ("PO\t" + "\t".join(COLUMNS) + "\n").encode()


class AverageError(ValueError):
    """a rejected input: ``name`` (the fragment or record it concerns) and ``path``"""

    def __init__(self, msg, name=None, path=None):
        ValueError.__init__(self, msg)
        self.name, self.path = name, path


# ---- windows ----------------------------------------------------------------------------------------------------------
def check_window(w, o):
    if int(w) < 2:
        raise ValueError("the window must be at least 2 (got %d)" % w)
    if not 0 <= int(o) < int(w):
        raise ValueError("the overlap must lie in [0, window) (got %d for window %d)" % (o, w))


def window_starts(lengths, w=WINDOW, o=OVERLAP):
    """fragment starts of records of ``lengths``: run_folding's range(-w/2, L - w/2, w - o) in Python 2 integer
    division (average_structure.py:47), i.e. from -ceil(w/2) up to L - floor(w/2), step w - o
    -> (record index int64 [F], start int64 [F]), records in order, starts ascending"""
    check_window(w, o)
    L = np.asarray(lengths, dtype=np.int64)
    first, step = -((w + 1) // 2), w - o
    stop = L - w // 2
    count = np.maximum(0, (stop - first + step - 1) // step)
    rec = np.repeat(np.arange(L.size, dtype=np.int64), count)
    base = np.zeros(L.size, dtype=np.int64)
    if L.size > 1:
        base[1:] = np.cumsum(count)[:-1]
    k = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(base, count)
    return rec, first + k * step


# ---- the value table --------------------------------------------------------------------------------------------------
def _triangle(n_max):
    n = np.repeat(np.arange(n_max + 1, dtype=np.int64), np.arange(1, n_max + 2))
    c = np.arange(n.size, dtype=np.int64) - n * (n + 1) // 2
    return c, n


@functools.lru_cache(maxsize=8)
def value_table(n_max, exact=False):
    """float64 [(n_max + 1)(n_max + 2) / 2]: entry n(n+1)/2 + c is c / n (``exact``) or what the scan reads for it from
    write_pfm's text: pandas' converter applied to ``repr(c / n)`` (pfmscan_profile_parse restates it bit for bit).
    Row n = 0 is never looked up (an uncovered position is an error) and holds 0."""
    from . import _lib
    c, n = _triangle(int(n_max))
    q = np.where(n > 0, c / np.maximum(n, 1), 0.0)
    if exact:
        return q
    text = "PO\tX\n" + "".join("0\t%r\n" % x for x in q.tolist())
    got = _lib.profile_parse(text.encode(), 1)
    if got is None or got.shape[0] != q.size:
        raise RuntimeError("the native profile parser refused the value table")
    got = np.ascontiguousarray(got[:, 0])
    got.setflags(write=False)
    return got


# ---- fragment input ---------------------------------------------------------------------------------------------------
def _map(path):
    with open(path, "rb") as f:
        if os.fstat(f.fileno()).st_size == 0:
            return None, np.zeros(0, dtype=np.uint8)
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    return mm, np.frombuffer(mm, dtype=np.uint8)


def _strings(buf, off, ln):
    """the (offset, length) spans of buf as str (ids: latin-1 keeps every byte)"""
    from . import _lib
    if len(off) == 0:
        return []
    blob = _lib.gather_spans(buf, np.stack([np.asarray(off, np.int64), np.asarray(ln, np.int64)], axis=1), 10)
    return blob.decode("latin-1").split("\n")[:-1]


def _gather(buf, off, ln, lut):
    """bytes buf[off[k], + ln[k]) of every span through lut, each followed by the separator -> (codes, offsets)"""
    from . import pack
    off, ln = np.asarray(off, np.int64), np.asarray(ln, np.int64)
    offsets = np.zeros(off.size, dtype=np.int64)
    if off.size > 1:
        offsets[1:] = np.cumsum(ln + 1)[:-1]
    total = int((ln + 1).sum())
    codes = np.full(total, pack.SEP, dtype=np.uint8)
    n = int(ln.sum())
    if n:
        within = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
        src = np.repeat(off, ln) + within
        dst = np.repeat(offsets, ln) + within
        codes[dst] = lut[buf[src]]
    return codes, offsets


class Fragments(object):
    """The fragments of a file, grouped by record (records in the order of their first appearance).

    ``ids`` record keys; ``lengths`` record lengths (the furthest fragment end); ``rec_frag`` [R + 1] file-order fragment
    ranges; per fragment (file order) ``names``-able id spans, ``start`` (the window start i), ``pos`` = max(i, 0) and
    ``flen`` (its letters).  ``encode(lo, hi)`` -> dot-bracket codes of fragments [lo, hi) in the stream layout."""

    def __init__(self, path, fmt="fasta"):
        from . import _lib
        if fmt not in ("fasta", "rnafold"):
            raise ValueError("fragment input must be 'fasta' or 'rnafold'")
        self.path, self.fmt = path, fmt
        self._mm, buf = _map(path)
        self.buf = buf
        if fmt == "fasta":
            hdr_off, hdr_len, seq_off, seq_end, n_letters = _lib.fasta_index(buf)
            self._seq = (seq_off, seq_end, n_letters)
            flen = n_letters
        else:
            hdr_off, hdr_len, s_off, s_len = self._rnafold_index(buf)
            self._seq = (s_off, s_len)
            flen = s_len
        spans, _ = _lib.fasta_ids(buf, hdr_off, hdr_len)
        self.id_spans = spans
        try:
            key_len, start = _lib.fragment_ids(buf, spans)
        except ValueError as e:
            k = getattr(e, "index", -1)
            name = self.fragment_name(k) if k >= 0 else None
            raise AverageError("fragment id %r (fragment %d of %s) does not end in _frag_<start>" % (name, k + 1, path),
                               name, path)
        keys = np.array(_strings(buf, spans[:, 0], key_len), dtype=object)
        F = keys.size
        new = np.ones(F, dtype=bool)
        if F > 1:
            new[1:] = keys[1:] != keys[:-1]
        first = np.flatnonzero(new)
        self.ids = keys[first].tolist()
        if len(set(self.ids)) != len(self.ids):
            seen = set()
            for r, rid in enumerate(self.ids):
                if rid in seen:
                    k = int(first[r])
                    raise AverageError("the fragments of record %r are not contiguous in %s (fragment %r, fragment %d of the "
                                       "file, follows another record's)" % (rid, path, self.fragment_name(k), k + 1),
                                       rid, path)
                seen.add(rid)
        self.rec_frag = np.append(first, F).astype(np.int64)
        self.start = start
        self.pos = np.maximum(start, 0)
        self.flen = np.asarray(flen, dtype=np.int64)
        rec = np.repeat(np.arange(len(self.ids), dtype=np.int64), np.diff(self.rec_frag))
        ends = self.pos + self.flen
        self.lengths = np.zeros(len(self.ids), dtype=np.int64)
        if F:
            np.maximum.at(self.lengths, rec, ends)
        self.rec_of = rec

    def fragment_name(self, k):
        return _strings(self.buf, self.id_spans[k:k + 1, 0], self.id_spans[k:k + 1, 1])[0]

    def _rnafold_index(self, buf):
        """RNAfold -p output: per record '>' header, sequence, MFE, ensemble, centroid, frequency line.  The structure is
        the first ' '-separated field of the fifth line (run_folding's get_centroid_from_RNAfold_output, :134-141).
        -> header spans, structure spans; a truncated record or a structure whose length differs from its sequence line
        is rejected, naming the record"""
        nl = np.flatnonzero(buf == 10)
        ls = np.concatenate([[0], nl + 1]).astype(np.int64)
        le = np.concatenate([nl, [buf.size]]).astype(np.int64)
        keep = ls < buf.size
        ls, le = ls[keep], le[keep]
        le = le - ((le > ls) & (buf[np.maximum(le - 1, 0)] == 13))        # \r\n line ends
        heads = np.flatnonzero(buf[ls] == ord(">"))
        nxt = np.append(heads[1:], ls.size)
        hdr_off, hdr_len = ls[heads] + 1, le[heads] - ls[heads] - 1
        short = np.flatnonzero(nxt - heads < 5)
        if short.size:
            from . import _lib
            r = int(short[0])
            spans, _ = _lib.fasta_ids(buf, hdr_off[r:r + 1], hdr_len[r:r + 1])
            name = _strings(buf, spans[:, 0], spans[:, 1])[0]
            raise AverageError("RNAfold record %r (record %d of %s) is truncated: fewer than the 5 lines header, sequence, "
                               "MFE, ensemble, centroid" % (name, r + 1, self.path), name, self.path)
        seq_len = le[heads + 1] - ls[heads + 1]
        c_off, c_end = ls[heads + 4], le[heads + 4]
        sp = np.flatnonzero(buf == ord(" "))                   # the structure ends at the first blank of its line
        if sp.size:
            at = np.minimum(np.searchsorted(sp, c_off), sp.size - 1)
            c_end = np.where((sp[at] >= c_off) & (sp[at] < c_end), sp[at], c_end)
        s_len = c_end - c_off
        bad = np.flatnonzero(s_len != seq_len)
        if bad.size:
            from . import _lib
            r = int(bad[0])
            spans, _ = _lib.fasta_ids(buf, hdr_off[r:r + 1], hdr_len[r:r + 1])
            name = _strings(buf, spans[:, 0], spans[:, 1])[0]
            raise AverageError("RNAfold record %r (record %d of %s): its centroid structure has %d characters, its sequence %d"
                               % (name, r + 1, self.path, int(s_len[r]), int(seq_len[r])), name, self.path)
        return hdr_off, hdr_len, c_off, s_len

    def encode(self, lo, hi):
        """dot-bracket codes of fragments [lo, hi) (file order), PFMSCAN_SEP after each -> (codes, offsets)"""
        from . import _lib
        if self.fmt == "fasta":
            seq_off, seq_end, n_letters = self._seq
            return _lib.fasta_encode(self.buf, seq_off, seq_end, n_letters, lo, hi, dotbracket.LUT)
        off, ln = self._seq
        return _gather(self.buf, off[lo:hi], ln[lo:hi], dotbracket.LUT)

    def batches(self, letters=BATCH_LETTERS):
        """contiguous record ranges of at most ``letters`` fragment letters (one record at least)"""
        cost = np.cumsum(self.flen + 1)
        per_rec = np.append(0, cost)[self.rec_frag]
        out, r, R = [], 0, len(self.ids)
        while r < R:
            e = int(np.searchsorted(per_rec, per_rec[r] + letters, side="right")) - 1
            e = min(max(e, r + 1), R)
            out.append((r, e))
            r = e
        return out


def _coverage_max(rec_row, n_rows, frag_row, frag_len):
    if frag_row.size == 0:
        return 0
    d = np.bincount(frag_row, minlength=n_rows + 1)[: n_rows + 1].astype(np.int64)
    d -= np.bincount(frag_row + frag_len, minlength=n_rows + 1)[: n_rows + 1]
    return int(np.cumsum(d).max())


def average_batch(ctx, frags, r0, r1, exact=False, dtype=np.float64, stats=None, stage=False):
    """records [r0, r1) of ``frags`` averaged on the device -> (rows [n_rows][7], rec_row int64 [r1 - r0]); with
    ``stage`` the rows stay staged in ctx's profile slot and None is returned for them"""
    from . import _lib
    t = time.perf_counter()
    f0, f1 = int(frags.rec_frag[r0]), int(frags.rec_frag[r1])
    codes, offsets = frags.encode(f0, f1)
    rec = frags.rec_of[f0:f1] - r0
    pos, flen = frags.pos[f0:f1], frags.flen[f0:f1]
    L = frags.lengths[r0:r1]
    rec_row = np.zeros(L.size, dtype=np.int64)
    if L.size > 1:
        rec_row[1:] = np.cumsum(L + 1)[:-1]
    n_rows = int((L + 1).sum())
    keep = flen > 0                                       # an empty fragment covers nothing
    order = np.lexsort((pos, rec))
    order = order[keep[order]]
    frag_off = offsets[order]
    frag_len = flen[order]
    frag_row = rec_row[rec[order]] + pos[order]
    rec_frag = np.zeros(L.size + 1, dtype=np.int64)
    rec_frag[1:] = np.cumsum(np.bincount(rec[order], minlength=L.size))
    cov = _coverage_max(rec_row, n_rows, frag_row, frag_len)
    n_max = max(1, min(cov, _lib.MAX_COVER))
    t1 = time.perf_counter()
    table = value_table(n_max, exact)
    t2 = time.perf_counter()
    try:
        if stage:
            ctx.average_stage(codes, frag_off, frag_len, frag_row, rec_row, L, rec_frag, table, n_max, dtype)
            rows = None
        else:
            rows = ctx.average_host(codes, frag_off, frag_len, frag_row, rec_row, L, rec_frag, table, n_max, dtype)
    except ValueError as e:
        kind = getattr(e, "kind", None)
        if kind is None:
            raise
        raise _named(frags, e, kind, f0, r0, offsets, rec_row)
    if stats is not None:
        stats["index"] = stats.get("index", 0.0) + (t1 - t)
        stats["table"] = stats.get("table", 0.0) + (t2 - t1)
        stats["device"] = stats.get("device", 0.0) + (time.perf_counter() - t2)
    return rows, rec_row


def _named(frags, e, kind, f0, r0, offsets, rec_row):
    from . import _lib
    p = int(e.position)
    if kind == _lib.AVG_DOTBRACKET:
        k = f0 + dotbracket.record_of(offsets, p)
        name = frags.fragment_name(k)
        return AverageError("invalid dot-bracket structure in fragment %r (fragment %d of %s, letter %d): unbalanced brackets "
                            "or a character outside '().'" % (name, k + 1, frags.path, p - int(offsets[k - f0]) + 1),
                            name, frags.path)
    if kind in (_lib.AVG_UNCOVERED, _lib.AVG_COVER):
        r = int(np.searchsorted(rec_row, p, side="right")) - 1
        rid = frags.ids[r0 + r]
        if kind == _lib.AVG_UNCOVERED:
            return AverageError("position %d of record %r (%s) is covered by no fragment" % (p - int(rec_row[r]) + 1, rid,
                                                                                            frags.path), rid, frags.path)
        return AverageError("position %d of record %r (%s) is covered by more than %d fragments"
                            % (p - int(rec_row[r]) + 1, rid, frags.path, _lib.MAX_COVER), rid, frags.path)
    return AverageError("%s (%s)" % (e, frags.path), None, frags.path)


# ---- output -----------------------------------------------------------------------------------------------------------
def build(ctx, frags_path, out, input_fmt="fasta", out_fmt="store", dtype=np.float64, stats=None, letters=BATCH_LETTERS):
    """average every record of a fragment file into ``out``: a packed store (store.ProfileStore opens it) or a directory
    of structure.<id>.txt files.  Returns the number of records."""
    from . import _lib
    t = time.perf_counter()
    frags = Fragments(frags_path, input_fmt)
    if stats is not None:
        stats["read"] = stats.get("read", 0.0) + time.perf_counter() - t
    dtype = np.dtype(dtype)
    if out_fmt == "text":
        bad = [rid for rid in frags.ids if "/" in rid]
        if bad:
            raise AverageError("record id %r of %s holds '/': it cannot name a structure.<id>.txt file" % (bad[0], frags_path),
                               bad[0], frags_path)
        dtype = np.dtype(np.float64)
    elif out_fmt != "store":
        raise ValueError("output format must be 'store' or 'text'")
    os.makedirs(out, exist_ok=True)
    name = "profile.f32" if dtype == np.float32 else "profile.f64"
    tmp = os.path.join(out, name + ".tmp")
    fh = open(tmp, "wb") if out_fmt == "store" else None
    scratch = [None]
    try:
        for r0, r1 in frags.batches(letters):
            rows, rec_row = average_batch(ctx, frags, r0, r1, exact=(out_fmt == "text"), dtype=dtype, stats=stats)
            t = time.perf_counter()
            if fh is not None:
                fh.write(rows.tobytes())
            else:
                _write_texts(out, frags.ids[r0:r1], frags.lengths[r0:r1], rows, rec_row, scratch)
            if stats is not None:
                stats["write"] = stats.get("write", 0.0) + time.perf_counter() - t
        if fh is not None:
            fh.close()
            fh = None
            os.replace(tmp, os.path.join(out, name))
            store.write_index(out, frags.ids, frags.lengths.tolist(), COLUMNS, dtype, name)
    finally:
        if fh is not None:
            fh.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    return len(frags.ids)


def _write_texts(out, ids, lengths, rows, rec_row, scratch):
    """write_pfm's text of every record of a batch (pfmutil.py:61-87): header, then `pos TAB 7 values` per row"""
    from . import _lib
    L = np.asarray(lengths, dtype=np.int64)
    keep = np.ones(rows.shape[0], dtype=bool)
    keep[rec_row + L] = False                                # the zero rows
    po = np.arange(rows.shape[0], dtype=np.int64) - np.repeat(rec_row, L + 1)
    vals = rows[keep]
    n = int(vals.shape[0])
    cols = [(_lib.TSV_I64, po[keep], None, None, 0)] + \
        [(_lib.TSV_F64, np.ascontiguousarray(vals[:, k]), None, None, 0) for k in range(7)]
    text = b"".join(bytes(p) for p in _lib.tsv_format(cols, n, estimate=n * 200 + 4096, scratch=scratch)) if n else b""
    ends = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1 if n else np.zeros(0, dtype=np.int64)
    line_end = np.concatenate([[0], ends])                  # byte offset after each line
    first_line = np.concatenate([[0], np.cumsum(L)])
    for r, rid in enumerate(ids):
        a, b = int(line_end[first_line[r]]), int(line_end[first_line[r + 1]])
        with open(os.path.join(out, "structure.%s.txt" % rid), "wb") as f:
            f.write(HEADER)
            f.write(text[a:b])


def built_store(ctx, frags_path, input_fmt="fasta", dtype=np.float64, directory=None):
    """the fragments averaged into a new temporary packed store -> its path (the caller removes it)"""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="rnascan_avg_", dir=directory)
    try:
        build(ctx, frags_path, d, input_fmt, "store", dtype)
    except BaseException:
        shutil.rmtree(d, ignore_errors=True)
        raise
    return d


# ---- the fragments command --------------------------------------------------------------------------------------------
def fragments_fasta(seqs_path, w=WINDOW, o=OVERLAP, min_length=MIN_LENGTH, batch_letters=1 << 26):
    """the FASTA run_folding feeds RNAfold: per record of at least ``min_length`` letters, one ``>id_frag_i`` record per
    window with the slice seq[max(i, 0) : i + w] as given -> yields bytes chunks"""
    from . import _lib
    check_window(w, o)
    mm, buf = _map(seqs_path)
    hdr_off, hdr_len, seq_off, seq_end, n_letters = _lib.fasta_index(buf)
    spans, _ = _lib.fasta_ids(buf, hdr_off, hdr_len)
    sel = np.flatnonzero(n_letters >= min_length)
    ident = np.arange(256, dtype=np.uint8)
    cost = np.cumsum(n_letters[sel] * (w // (w - o) + 2) + 1)      # ~ output bytes per record
    a = 0
    while a < sel.size:
        b = int(np.searchsorted(cost, (cost[a - 1] if a else 0) + batch_letters, side="right"))
        b = min(max(b, a + 1), sel.size)
        recs = sel[a:b]
        yield _fragment_chunk(buf, spans[recs], seq_off, seq_end, n_letters, recs, ident, w, o)
        a = b


def _fragment_chunk(buf, spans, seq_off, seq_end, n_letters, recs, ident, w, o):
    from . import _lib
    letters = []
    offs = []
    for lo, hi in _runs(recs):
        c, of = _lib.fasta_encode(buf, seq_off, seq_end, n_letters, lo, hi, ident, separator=10)
        offs.append(of + sum(x.size for x in letters))
        letters.append(c)
    seq = np.concatenate(letters) if letters else np.zeros(0, np.uint8)
    rec_off = np.concatenate(offs) if offs else np.zeros(0, np.int64)
    L = n_letters[recs]
    rec, start = window_starts(L, w, o)
    lo = np.maximum(start, 0)
    hi = np.minimum(start + w, L[rec])
    flen = np.maximum(hi - lo, 0)
    ids = np.array(_strings(buf, spans[:, 0], spans[:, 1]), dtype=object)
    heads = (np.char.add(np.char.add(np.char.add(">", ids[rec].astype(str)), "_frag_"), start.astype(str)))
    hb = np.char.encode(heads, "latin-1")
    W = hb.dtype.itemsize
    hl = np.char.str_len(hb).astype(np.int64) if hb.size else np.zeros(0, np.int64)
    seg = hl + 1 + flen + 1
    base = np.zeros(seg.size, dtype=np.int64)
    if seg.size > 1:
        base[1:] = np.cumsum(seg)[:-1]
    out = np.empty(int(seg.sum()), dtype=np.uint8)
    if hb.size:
        hbytes = np.frombuffer(hb.tobytes(), dtype=np.uint8).reshape(hb.size, W)
        j = np.arange(W)
        m = j[None, :] < hl[:, None]
        out[(base[:, None] + j[None, :])[m]] = hbytes[m]
    out[base + hl] = 10
    out[base + seg - 1] = 10
    n = int(flen.sum())
    if n:
        within = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(flen) - flen, flen)
        out[np.repeat(base + hl + 1, flen) + within] = seq[np.repeat(rec_off[rec] + lo, flen) + within]
    return out.tobytes()


def _runs(idx):
    """consecutive runs of a sorted index array -> [(lo, hi)]"""
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) != 1) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [idx.size]])
    return [(int(idx[s]), int(idx[e - 1]) + 1) for s, e in zip(starts, ends)]


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.average",
                                     description="Averaged-structure profiles from fragment structures (the averaging of the "
                                                 "reference's run_folding, on the GPU; folding itself stays outside).")
    sub = parser.add_subparsers(dest="cmd", required=True)
    fr = sub.add_parser("fragments", help="write the windows run_folding folds as FASTA to STDOUT")
    fr.add_argument("fasta")
    fr.add_argument("-w", "--window", type=int, default=WINDOW, help="window length [%(default)s]")
    fr.add_argument("-o", "--overlap", type=int, default=OVERLAP, help="overlap of consecutive windows [%(default)s]")
    fr.add_argument("--min-length", type=int, default=MIN_LENGTH, help="skip shorter records [%(default)s]")
    bu = sub.add_parser("build", help="average fragment structures into a packed store or structure.<id>.txt files")
    bu.add_argument("frags", help="fragment structures: FASTA of dot-bracket strings named <id>_frag_<i>, or RNAfold -p output")
    bu.add_argument("out", help="the store directory, or the directory of text files")
    bu.add_argument("--input", choices=["fasta", "rnafold"], default="fasta", help="[%(default)s]")
    bu.add_argument("--format", choices=["store", "text"], default="store", help="[%(default)s]")
    bu.add_argument("--dtype", choices=["float64", "float32"], default="float64", help="store rows [%(default)s]")
    bu.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")
    args = parser.parse_args(argv)
    if args.cmd == "fragments":
        try:
            check_window(args.window, args.overlap)
        except ValueError as e:
            parser.error(str(e))
        out = sys.stdout.buffer
        for chunk in fragments_fasta(args.fasta, args.window, args.overlap, args.min_length):
            out.write(chunk)
        out.flush()
        return 0
    from . import _lib
    with _lib.Context(args.device) as ctx:
        try:
            n = build(ctx, args.frags, args.out, args.input, args.format, np.dtype(args.dtype))
        except AverageError as e:
            fasta.eprint(str(e))
            return 1
    fasta.eprint("Averaged %d records into %s" % (n, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
