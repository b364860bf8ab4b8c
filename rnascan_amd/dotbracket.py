"""Dot-bracket structure input: ``((..((...))..))`` -> the structure-context letters EHTBLRM, annotated on the GPU.

Replaces the reference's separate binary scripts/parse_secondary_structure.cpp (run by hand, one line at a time, before
any structure-letter scan).  The annotation itself is the kernels of csrc/pfmscan_dotbracket.hip behind
``pfmscan_dotbracket_*`` (include/pfmscan.h, where the rules are written out); this module holds the host side:

  - ``LUT``: bytes -> dot-bracket codes ('.' 0, '(' 1, ')' 2, anything else 3) for ``pfmscan_fasta_encode``;
  - ``detect``: is a structure FASTA dot-bracket or letters;
  - ``annotate_fasta``: a FASTA of dot-bracket records -> the same records as letters (headers kept, one sequence line
    per record), with rejected records named by id and file;
  - ``python -m rnascan_amd.dotbracket in.fa > out.fa``: that conversion as a command, the drop-in for the binary.

Deviation from the reference: a record with unbalanced brackets or a character outside ``().`` (pseudoknot brackets,
blanks inside the string, RNAfold's energy field) is rejected with an error naming it.  The reference's parser reads past
the end of such a string or silently drops what it does not know.
"""
import argparse
import os
import sys

import numpy as np

from . import fasta, pack

DOT, OPEN, CLOSE, OTHER = 0, 1, 2, 3

LUT = np.full(256, OTHER, dtype=np.uint8)
LUT[ord(".")] = DOT
LUT[ord("(")] = OPEN
LUT[ord(")")] = CLOSE

# detection: brackets, dots, structure letters (either case) and everything else, counted over record bodies
_LETTER = 4
_DETECT_LUT = LUT.copy()
for _ch in pack.STRUCT_LETTERS:
    _DETECT_LUT[ord(_ch)] = _LETTER
    _DETECT_LUT[ord(_ch.lower())] = _LETTER

# annotated codes (EHTBLRM indices, separator) -> the bytes of the converted FASTA: letters, '\n' after every record
_ASCII = np.full(256, ord("?"), dtype=np.uint8)
for _i, _ch in enumerate(pack.STRUCT_LETTERS):
    _ASCII[_i] = ord(_ch)
_ASCII[pack.SEP] = ord("\n")

BATCH_POSITIONS = 1 << 28          # positions annotated per launch sequence (device scratch ~11 bytes per position)


class DotBracketError(ValueError):
    """a rejected record: ``record_id``, ``record`` (0-based index in the file), ``path``"""

    def __init__(self, msg, record_id=None, record=None, path=None):
        ValueError.__init__(self, msg)
        self.record_id, self.record, self.path = record_id, record, path


def _packed_batches(lazy, lut, positions):
    """(lo, hi, codes, offsets) per batch of records: the native packer, or -- for compressed / CR-only files, which
    LazyFasta parses in Python -- the records' strings through the same LUT"""
    from . import shard
    for lo, hi in shard.batches(lazy.lengths, 0, len(lazy), positions):
        if hi <= lo:
            continue
        packed = lazy[lo:hi].pack_letters(lut)
        if packed is None:
            recs = lazy[lo:hi]
            s = pack.pack([lut[np.frombuffer(r.seq.encode("latin-1", "replace"), dtype=np.uint8)] for r in recs])
            packed = (s.codes, s.offsets, s.lengths)
        yield lo, hi, packed[0], packed[1]


def body_counts(path, lut=_DETECT_LUT, positions=1 << 26):
    """int64 [256]: how often each code of ``lut`` occurs in the record bodies of a FASTA (headers not counted; one
    separator per record counted under pack.SEP)"""
    from . import _lib
    lazy = fasta.open_lazy(path)
    counts = np.zeros(256, dtype=np.int64)
    for _, _, codes, _ in _packed_batches(lazy, lut, positions):
        counts += _lib.count_bytes(codes)
    return counts


def detect(path):
    """"dotbracket" when the record bodies of the FASTA hold at least one '(' and no structure letter (EHTBLRM in either
    case) -- files of '(' ')' '.' only, and folding output with extra fields, which the annotation then rejects by
    record; otherwise "letters".  A dot-only file is "letters" (its letters path and its annotation agree: all E).  The
    rule reads record bodies only: a header may hold anything."""
    c = body_counts(path)
    return "dotbracket" if c[OPEN] > 0 and c[_LETTER] == 0 else "letters"


def has_brackets(path):
    """True when some record body of the FASTA holds '(' or ')'"""
    c = body_counts(path)
    return bool(c[OPEN] or c[CLOSE])


def is_dotbracket_string(s):
    """the -t form: a structure string is dot-bracket when it holds a '(' and no structure letter"""
    b = _DETECT_LUT[np.frombuffer(s.encode("latin-1", "replace"), dtype=np.uint8)]
    return bool(np.any(b == OPEN)) and not bool(np.any(b == _LETTER))


def record_of(offsets, position):
    """index of the record (within a packed batch) that holds stream ``position``; a record's separator belongs to it"""
    return int(np.searchsorted(np.asarray(offsets, dtype=np.int64), int(position), side="right")) - 1


def annotate_fasta(ctx, path, positions=BATCH_POSITIONS):
    """every record of a dot-bracket FASTA annotated on the device -> (list of bytes chunks of the converted FASTA:
    '>' header, newline, the letters, newline, per record; int64 [7] counts of E H T B L R M).  Nothing is returned
    for a file with a rejected record: DotBracketError names the first one."""
    lazy = fasta.open_lazy(path)
    chunks = []
    total = np.zeros(7, dtype=np.int64)
    for lo, hi, codes, offsets in _packed_batches(lazy, LUT, positions):
        try:
            out, counts = ctx.dotbracket_annotate_host(codes)
        except ValueError as e:
            pos = getattr(e, "position", None)
            if pos is None:
                raise
            k = lo + record_of(offsets, pos)
            rid = lazy.ids[k]
            raise DotBracketError("invalid dot-bracket structure in record %r (record %d of %s, letter %d): %s"
                                  % (rid, k + 1, path, int(pos - offsets[k - lo]) + 1,
                                     "unbalanced brackets or a character outside '().'"), rid, k, path)
        total += counts
        body = _ASCII[out].tobytes()                 # "letters\n" per record, back to back
        heads = lazy.headers.tolist(lo, hi)
        ends = np.asarray(offsets, dtype=np.int64) - offsets[0] if len(offsets) else offsets
        mv = memoryview(body)
        for r, h in enumerate(heads):
            a = int(ends[r])
            b = int(ends[r + 1]) if r + 1 < len(heads) else len(body)
            chunks.append((">" + h + "\n").encode("utf-8", "surrogateescape"))
            chunks.append(mv[a:b])
    return chunks, total


def annotated_copy(ctx, path, directory=None):
    """annotate_fasta(path) written to a new temporary file -> its path (the caller removes it)"""
    import tempfile
    chunks, _ = annotate_fasta(ctx, path)
    fd, tmp = tempfile.mkstemp(prefix="rnascan_struct_", suffix=".fa", dir=directory)
    try:
        with os.fdopen(fd, "wb") as f:
            f.writelines(chunks)
    except BaseException:
        os.remove(tmp)
        raise
    return tmp


def annotate_string(ctx, s):
    """one dot-bracket string -> its letters (the -t form)"""
    codes = np.append(LUT[np.frombuffer(s.encode("latin-1", "replace"), dtype=np.uint8)], np.uint8(pack.SEP))
    try:
        out, _ = ctx.dotbracket_annotate_host(codes)
    except ValueError as e:
        if getattr(e, "position", None) is None:
            raise
        raise DotBracketError("invalid dot-bracket structure %r (letter %d): unbalanced brackets or a character outside "
                              "'().'" % (s, int(e.position) + 1))
    return _ASCII[out[:-1]].tobytes().decode("ascii")


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rnascan_amd.dotbracket",
                                     description=("Annotate dot-bracket structures with their structural context letters "
                                                  "(EHTBLRM) on the GPU.  Writes FASTA to STDOUT: headers kept, one line of "
                                                  "letters per record."))
    parser.add_argument("fasta", help="FASTA of dot-bracket structures")
    parser.add_argument("--device", type=int, default=int(os.environ.get("RNASCAN_DEVICE", "0")), help="HIP device index [%(default)s]")
    args = parser.parse_args(argv)
    from . import _lib
    with _lib.Context(args.device) as ctx:
        try:
            chunks, _ = annotate_fasta(ctx, args.fasta)
        except DotBracketError as e:
            fasta.eprint(str(e))
            return 1
    out = sys.stdout.buffer
    out.writelines(chunks)
    out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
