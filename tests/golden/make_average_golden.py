#!/usr/bin/env python3
"""Regenerate tests/golden/average/ -- runs ONLY in the build container, where the upstream checkout is mounted read-only
at /root/reference.  CPU only; the GPU box never sees the reference, it gets the data files this writes.

What is captured, per window / overlap pair (100, 95), (40, 30), (101, 0), (7, 3):

  - seeded random RNA records of 30 .. 900 nt (records of 50 nt or less are kept in the sequence file: run_folding skips
    them, :63-65, and so must the fragments command);
  - their fragments, cut as run_folding cuts them: starts range(-w/2, L - w/2, w - o) in PYTHON 2 integer division
    (average_structure.py:47: -w/2 is floor(-w/2) = -ceil(w/2), L - w/2 is L - floor(w/2)), fragment i is
    seq[max(i, 0) : i + w] named <id>_frag_<i> (:52-59);
  - a random structure of each fragment's length with at least one '.' (tests/dotbracket_rules.random_structure), in
    place of RNAfold's centroid;
  - the structures annotated by the reference's parse_secondary_structure (compiled with g++ into a temporary
    directory that is removed afterwards -- nothing of it is kept), aligned as average_structure.py:89-92 aligns them,
    counted, normalised and formatted by the reference's own struct_pfm_from_aligned, norm_pfm and format_pfm (imported
    with empty Bio placeholders: Biopython is not installed here, and no Biopython code is used by those functions).

A record whose alignment leaves a position uncovered makes the reference divide by zero (norm_pfm); such records are
left out of the fragment and profile files (this project rejects them, naming the position).

Files (gzip):
  seqs_w<w>_o<o>.fa.gz        the records (one line each)
  frags_w<w>_o<o>.fa.gz       the fragment structures, >id_frag_i + dot-bracket, in run_folding's order
  profiles_w<w>_o<o>.txt.gz   per record: a line "=structure.<id>.txt", then that file's bytes

Run:  python3 -B tests/golden/make_average_golden.py
"""
import gzip
import importlib
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dotbracket_rules import random_structure  # noqa: E402

REF = "/root/reference"
REF_SRC = os.path.join(REF, "scripts", "parse_secondary_structure.cpp")
OUT = os.path.join(HERE, "average")
PAIRS = [(100, 95), (40, 30), (101, 0), (7, 3)]
N_RECORDS = {(100, 95): 10, (40, 30): 12, (101, 0): 14, (7, 3): 10}


def py2_starts(L, w, o):
    """range(-w/2, L - w/2, w - o) with Python 2's integer division (floor for ints)"""
    return list(range(-((w + 1) // 2), L - w // 2, w - o))


def reference_functions():
    for name in ("Bio", "Bio.SeqIO", "Bio.SeqRecord", "Bio.Seq"):
        m = types.ModuleType(name)
        m.SeqRecord, m.Seq = object, object
        sys.modules[name] = m
    sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
    sys.path.insert(0, REF)
    avg = importlib.import_module("rnascan.average_structure")
    pfmutil = importlib.import_module("rnascan.pfmutil")
    return avg.struct_pfm_from_aligned, pfmutil.norm_pfm, pfmutil.format_pfm


def main():
    if not os.path.exists(REF_SRC):
        sys.exit("the reference checkout is not here (%s); fixtures are regenerated in the build container only" % REF_SRC)
    count, norm, fmt = reference_functions()
    rng = np.random.default_rng(20261016)
    plan = []                  # (w, o, [(id, seq, [(start, structure)])])
    for w, o in PAIRS:
        recs = []
        for r in range(N_RECORDS[(w, o)]):
            L = int(rng.integers(30, 901)) if r > 1 else (30 if r == 0 else int(rng.integers(51, 120)))
            seq = "".join(rng.choice(list("ACGU"), size=L))
            frags = []
            for i in py2_starts(L, w, o):
                n = len(seq[max(i, 0):i + w])
                s = random_structure(rng, n)
                while "." not in s:
                    s = random_structure(rng, n)
                frags.append((i, s))
            recs.append(("w%do%d_r%02d" % (w, o, r), seq, frags))
        plan.append((w, o, recs))
    tmp = tempfile.mkdtemp(prefix="average_ref_")
    try:
        exe = os.path.join(tmp, "parse_secondary_structure")
        subprocess.check_call(["g++", "-O2", "-o", exe, REF_SRC])
        lines = [s for _, _, recs in plan for _, _, frags in recs for _, s in frags]
        inp, outp = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(inp, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call([exe, inp, outp])
        with open(outp) as f:
            letters = f.read().split("\n")[:len(lines)]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(letters) == len(lines)
    os.makedirs(OUT, exist_ok=True)
    k = 0
    for w, o, recs in plan:
        seqs, frag_lines, profiles, skipped = [], [], [], 0
        for rid, seq, frags in recs:
            seqs.append(">%s\n%s\n" % (rid, seq))
            ann = letters[k:k + len(frags)]
            k += len(frags)
            if len(seq) <= 50:                                      # run_folding:63-65
                continue
            aligned = ["-" * i + a.rstrip() + "-" * (len(seq) - (i + w)) for (i, _), a in zip(frags, ann)]  # :89-92
            try:
                text = fmt(norm(count(aligned)))
            except ZeroDivisionError:
                skipped += 1
                continue
            frag_lines.extend(">%s_frag_%d\n%s\n" % (rid, i, s) for i, s in frags)
            profiles.append("=structure.%s.txt\n%s" % (rid, text))
        for name, body in (("seqs_w%d_o%d.fa.gz" % (w, o), seqs), ("frags_w%d_o%d.fa.gz" % (w, o), frag_lines),
                           ("profiles_w%d_o%d.txt.gz" % (w, o), profiles)):
            with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
                f.write("".join(body).encode("ascii"))
        print("w=%d o=%d: %d records, %d with profiles, %d left out (uncovered positions)"
              % (w, o, len(recs), len(profiles), skipped))


if __name__ == "__main__":
    main()
