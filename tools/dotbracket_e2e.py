"""Dot-bracket input at C3 size on the GPU box: R synthetic structures x L positions written as a dot-bracket FASTA and as
the letters FASTA of the same records (the reference's parse_secondary_structure output, by tests/dotbracket_rules.py),
then `rnascan -q pfm dot.fa` against `rnascan -q pfm letters.fa` (with -u and with the default background): wall times
and the check that the two tables are the same bytes.

usage: python tools/dotbracket_e2e.py [--records R] [--length L] [--dir D] [--write-only] [--annotate-only N]
  --write-only     write the two FASTA files (and structures.txt, one structure per line) into --dir and stop
  --annotate-only  no files and no command line: annotate the packed stream N times on the device (for rocprofv3)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

from dotbracket_rules import annotate, random_structure  # noqa: E402

STRUCT_PFM = os.path.join(REPO, "tests", "golden", "data", "SLBP_pfm_assembled_normalized_struct.txt")


def records(R, L, seed=0, pool=64, head=100):
    """R records: one of 256 random heads of `head` positions + one of `pool` random bodies -> (pools, pick arrays)"""
    rng = np.random.default_rng(seed)
    heads = [random_structure(rng, head) for _ in range(256)]
    bodies = [random_structure(rng, L - head) for _ in range(pool)]
    return heads, bodies, rng.integers(0, 256, size=R), rng.integers(0, pool, size=R)


def write_files(d, R, L):
    heads, bodies, hw, bw = records(R, L)
    ah, ab = [annotate(x) for x in heads], [annotate(x) for x in bodies]
    paths = {k: os.path.join(d, k) for k in ("dot.fa", "letters.fa", "structures.txt")}
    with open(paths["dot.fa"], "w") as f, open(paths["letters.fa"], "w") as g, open(paths["structures.txt"], "w") as s:
        for i in range(R):
            f.write(">t%d structure %d\n%s%s\n" % (i, i, heads[hw[i]], bodies[bw[i]]))
            g.write(">t%d structure %d\n%s%s\n" % (i, i, ah[hw[i]], ab[bw[i]]))
            s.write("%s%s\n" % (heads[hw[i]], bodies[bw[i]]))
    return paths


def annotate_only(R, L, n):
    from rnascan_amd import _lib, dotbracket
    heads, bodies, hw, bw = records(R, L)
    hc = np.stack([dotbracket.LUT[np.frombuffer(x.encode(), dtype=np.uint8)] for x in heads])
    bc = np.stack([dotbracket.LUT[np.frombuffer(x.encode(), dtype=np.uint8)] for x in bodies])
    view = np.full((R, L + 1), 7, dtype=np.uint8)
    view[:, :100] = hc[hw]
    view[:, 100:L] = bc[bw]
    import torch
    d_in = torch.from_numpy(view.reshape(-1)).to("cuda:0")
    d_out = torch.empty_like(d_in)
    d_counts = torch.zeros(7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with _lib.Context(0) as ctx:
        times = []
        for _ in range(n):
            ctx.synchronize()
            t = time.perf_counter()
            ctx.dotbracket_annotate_dev(d_in, d_out, d_in.numel(), d_counts=d_counts)
            ctx.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
    print(json.dumps({"positions": int(d_in.numel()), "annotate_wall_ms": [round(x, 3) for x in times],
                      "counts": d_counts.cpu().tolist()}))


def run(cmd):
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True)
    dt = time.perf_counter() - t
    if r.returncode:
        sys.exit("failed: %s\n%s" % (" ".join(cmd), r.stderr.decode()[-3000:]))
    return dt, hashlib.sha256(r.stdout).hexdigest(), r.stdout.count(b"\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--annotate-only", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    if a.annotate_only:
        annotate_only(a.records, a.length, a.annotate_only)
        return
    d = a.dir or tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    os.makedirs(d, exist_ok=True)
    t = time.perf_counter()
    paths = write_files(d, a.records, a.length)
    print(json.dumps({"wrote": d, "seconds": round(time.perf_counter() - t, 2)}), flush=True)
    if a.write_only:
        return
    rnascan = [sys.executable, os.path.join(REPO, "bin", "rnascan"), "-q", STRUCT_PFM]
    for label, extra in (("uniform", ["-u"]), ("default_background", [])):
        res = {}
        for kind in ("letters.fa", "dot.fa"):
            runs = [run(rnascan + extra + [paths[kind]]) for _ in range(a.repeat)]
            res[kind] = {"wall_s": [round(x[0], 3) for x in runs], "sha256": runs[0][1], "lines": runs[0][2]}
        same = res["letters.fa"]["sha256"] == res["dot.fa"]["sha256"]
        ratio = min(res["dot.fa"]["wall_s"]) / min(res["letters.fa"]["wall_s"])
        print(json.dumps({"case": label, "records": a.records, "length": a.length, "same_bytes": same,
                          "ratio_dot_over_letters": round(ratio, 3), **res}), flush=True)
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
