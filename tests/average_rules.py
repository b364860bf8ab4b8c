"""A numpy restatement of the reference's averaging (rnascan/average_structure.py:89-92 alignment, struct_pfm_from_aligned
:28-42, norm_pfm and write_pfm in pfmutil.py:136-151, :61-87), pinned to the reference's output by the goldens of
tests/golden/average/ (test_average_cpu.py), and the readers of those goldens."""
import gzip
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "average")
PAIRS = [(100, 95), (40, 30), (101, 0), (7, 3)]
COLUMNS = "BEHLMRT"
# letter -> column in B E H L M R T
COLUMN_OF = {ch: COLUMNS.index(ch) for ch in COLUMNS}


def py2_starts(L, w, o):
    """range(-w/2, L - w/2, w - o) as Python 2 evaluates it (integer division floors)"""
    return list(range(-((w + 1) // 2), L - w // 2, w - o))


def counts(pos, letters, L=None):
    """fragments (first covered position max(i, 0), their EHTBLRM letters) -> int64 [L][7] counts in B E H L M R T order;
    L defaults to the furthest fragment end"""
    L = max((p + len(s) for p, s in zip(pos, letters)), default=0) if L is None else L
    c = np.zeros((L, 7), dtype=np.int64)
    lut = np.full(256, 7, dtype=np.int64)
    for ch, k in COLUMN_OF.items():
        lut[ord(ch)] = k
    for p, s in zip(pos, letters):
        k = lut[np.frombuffer(s.encode(), dtype=np.uint8)]
        np.add.at(c, (np.arange(p, p + len(s)), k), 1)
    return c


def values(c):
    """c / n per row in fp64 (norm_pfm); ZeroDivisionError where a row is uncovered, as the reference"""
    n = c.sum(axis=1, keepdims=True)
    if np.any(n == 0):
        raise ZeroDivisionError("uncovered position")
    return c / n


def text(c):
    """write_pfm's bytes for count rows c"""
    v = values(c)
    out = ["PO\t" + "\t".join(COLUMNS) + "\n"]
    for i, row in enumerate(v.tolist()):
        out.append(str(i) + "".join("\t" + str(x) for x in row) + "\n")
    return "".join(out).encode()


def scanned(c):
    """what the scan reads back from text(c): pandas' parse of str(c / n) (its converter, restated natively)"""
    from rnascan_amd import _lib
    return _lib.profile_parse(text(c), 7)


def read_fasta_gz(path):
    """[(id, body)] of a one-line-per-record FASTA"""
    with gzip.open(path, "rt") as f:
        lines = f.read().split("\n")
    return [(lines[k][1:], lines[k + 1]) for k in range(0, len(lines) - 1, 2)]


def golden(w, o):
    """(sequences [(id, seq)], fragments [(name, structure)], {file name: bytes})"""
    seqs = read_fasta_gz(os.path.join(GOLDEN, "seqs_w%d_o%d.fa.gz" % (w, o)))
    frags = read_fasta_gz(os.path.join(GOLDEN, "frags_w%d_o%d.fa.gz" % (w, o)))
    with gzip.open(os.path.join(GOLDEN, "profiles_w%d_o%d.txt.gz" % (w, o)), "rb") as f:
        blob = f.read()
    texts = {}
    for part in blob.split(b"=structure.")[1:]:
        head, body = part.split(b"\n", 1)
        texts["structure." + head.decode()] = body
    return seqs, frags, texts


def golden_fasta_path(tmp_path, w, o, kind="frags"):
    """the golden FASTA unzipped into tmp_path"""
    src = os.path.join(GOLDEN, "%s_w%d_o%d.fa.gz" % (kind, w, o))
    dst = os.path.join(str(tmp_path), "%s_w%d_o%d.fa" % (kind, w, o))
    with gzip.open(src, "rb") as f, open(dst, "wb") as g:
        g.write(f.read())
    return dst


def split_name(name):
    key, _, start = name.rpartition("_frag_")
    return key, int(start)
