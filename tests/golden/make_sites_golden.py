#!/usr/bin/env python3
"""Regenerate tests/golden/sites/ -- runs ONLY in the build container, where the upstream checkout is mounted read-only at
/root/reference.  CPU only; the GPU box never sees the reference, it gets the data file this writes.

What is captured: seeded random records (a nucleotide string and a structure-letter string of the same length each), a
seeded list of sites (record, 0-based start) of width m, and -- for flank 0 and flank 3 -- the structure PFM of the aligned
site windows as the reference makes one: the windows (columns over a record end written as '-', which
struct_pfm_from_aligned skips, average_structure.py:28-42) counted by the reference's own struct_pfm_from_aligned and
normalised by its norm_pfm (pfmutil.py:136-151), both imported with empty Bio placeholders: Biopython is not installed
here, and no Biopython code is used by those functions.  One record holds more than 4096 sites.

File (gzip JSON): sites.json.gz  {"m", "records": [[id, seq, struct]], "sites": [[record index, start]],
                                  "pfm": {"0": {letter: [hex floats]}, "3": {...}}, "counts": {"0": {letter: [ints]}, ...}}

Run:  python3 -B tests/golden/make_sites_golden.py
"""
import gzip
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "sites")
M = 9
FLANKS = (0, 3)


def reference_functions():
    for name in ("Bio", "Bio.SeqIO", "Bio.SeqRecord", "Bio.Seq"):
        m = types.ModuleType(name)
        m.SeqRecord, m.Seq = object, object
        sys.modules[name] = m
    sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
    sys.path.insert(0, REF)
    avg = importlib.import_module("rnascan.average_structure")
    pfmutil = importlib.import_module("rnascan.pfmutil")
    return avg.struct_pfm_from_aligned, pfmutil.norm_pfm


def main():
    if not os.path.exists(os.path.join(REF, "rnascan", "average_structure.py")):
        sys.exit("the reference checkout is not here (%s); fixtures are regenerated in the build container only" % REF)
    count, norm = reference_functions()
    rng = np.random.default_rng(20261019)
    records, sites = [], []
    for r in range(24):
        L = 4200 + M if r == 5 else (M if r == 0 else (M + 1 if r == 1 else int(rng.integers(M, 300))))
        seq = "".join(rng.choice(list("ACGU"), size=L))
        struct = "".join(rng.choice(list("BEHLMRT"), size=L, p=[.05, .3, .15, .2, .05, .15, .1]))
        records.append(["rec%d" % r, seq, struct])
        starts = np.arange(L - M + 1)
        keep = starts if r in (0, 1, 5) else starts[rng.random(starts.size) < 0.08]
        if r not in (0, 1, 5) and starts.size:
            keep = np.union1d(keep, [0, starts[-1]])            # the record's first and last window
        sites += [[r, int(s)] for s in keep]
    pfm, counts = {}, {}
    for F in FLANKS:
        aligned = []
        for r, s in sites:
            st = records[r][2]
            aligned.append("".join(st[x] if 0 <= x < len(st) else "-" for x in range(s - F, s + M + F)))
        c = count(aligned)
        p = norm(c)
        counts[str(F)] = {k: [int(x) for x in v] for k, v in c.items()}
        pfm[str(F)] = {k: [float(x).hex() for x in v] for k, v in p.items()}
    os.makedirs(OUT, exist_ok=True)
    with gzip.GzipFile(os.path.join(OUT, "sites.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps({"m": M, "records": records, "sites": sites, "pfm": pfm, "counts": counts}, sort_keys=True).encode("ascii"))
    print("wrote %d records, %d sites" % (len(records), len(sites)))


if __name__ == "__main__":
    main()
