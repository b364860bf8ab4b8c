#!/usr/bin/env python3
"""Regenerate tests/golden/dotbracket/ -- runs ONLY in the build container, where the upstream checkout is mounted
read-only at /root/reference.  CPU only; the GPU box never sees the reference, it gets the data files this writes.

What is captured: the reference's dot-bracket parser (scripts/parse_secondary_structure.cpp, compiled with g++ into a
temporary directory that is removed afterwards -- nothing of it is kept) run once over

  - about 2 000 seeded random structures, lengths 1 .. 3000 (log-uniform), stems, hairpins, bulges, interior loops
    and multiloops at varied pairing densities (tests/dotbracket_rules.random_structure);
  - the hand cases of the issue that introduced dot-bracket input;
  - a few deep (depth >= 500) and long-range (a pair spanning more than 10 kb) structures.

Files (gzip text, one structure per line, the same order in both):
  structures.txt.gz   the input lines
  reference.txt.gz    the reference binary's output lines

The binary's ``main`` skips input lines without a '.', so every structure here holds at least one dot.

Run:  python3 -B tests/golden/make_dotbracket_golden.py
"""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/: the rules module and its generator
from dotbracket_rules import annotate, deep_structure, random_structure  # noqa: E402

REF_SRC = "/root/reference/scripts/parse_secondary_structure.cpp"
OUT = os.path.join(HERE, "dotbracket")

HAND = ["(((...)))", "..((..))..((..))..", "((..((...))..((...))..))", "(.(...).)", "((.(...)))", "(((...)).)", ".", "...",
        "(...)((...))"]


def structures(seed=20261015, n_random=2000):
    rng = np.random.default_rng(seed)
    out = list(HAND)
    while len(out) < len(HAND) + n_random:
        n = int(np.exp(rng.uniform(0.0, np.log(3000.0)))) if rng.random() < 0.8 else int(rng.integers(1, 3001))
        s = random_structure(rng, max(1, min(n, 3000)))
        if "." in s:
            out.append(s)
    # deep: one stem of 600 pairs; a deep stem around a random multiloop body; long-range: pairs spanning > 10 kb
    out.append(deep_structure(600))
    out.append("(" * 512 + random_structure(rng, 2000, 0.6) + ")" * 512 + "..")
    out.append("." + "(" + random_structure(rng, 12000, 0.5) + ")" + "((" + random_structure(rng, 15000, 0.3) + "))")
    out.append("((" + random_structure(rng, 11000, 0.7) + "..)).(" + "." * 10500 + ")")
    assert all("." in s for s in out)
    return out


def main():
    if not os.path.exists(REF_SRC):
        sys.exit("the reference checkout is not here (%s); fixtures are regenerated in the build container only" % REF_SRC)
    structs = structures()
    tmp = tempfile.mkdtemp(prefix="dotbracket_ref_")
    try:
        exe = os.path.join(tmp, "parse_secondary_structure")
        subprocess.check_call(["g++", "-O2", "-o", exe, REF_SRC])
        inp, outp = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(inp, "w") as f:
            f.write("\n".join(structs) + "\n")
        subprocess.check_call([exe, inp, outp])
        with open(outp) as f:
            got = f.read().split("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    got = got[:len(structs)]
    assert len(got) == len(structs), "the reference wrote %d lines for %d structures" % (len(got), len(structs))
    bad = [i for i, (s, r) in enumerate(zip(structs, got)) if annotate(s) != r]
    print("%d structures, restatement differs on %d" % (len(structs), len(bad)))
    os.makedirs(OUT, exist_ok=True)
    for name, lines in (("structures.txt.gz", structs), ("reference.txt.gz", got)):
        with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
            f.write(("\n".join(lines) + "\n").encode("ascii"))
    if bad:
        sys.exit("the restatement (tests/dotbracket_rules.py) disagrees with the reference on %d structures, e.g. #%d"
                 % (len(bad), bad[0]))


if __name__ == "__main__":
    main()
