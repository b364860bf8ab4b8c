"""`python -m rnascan_amd.expect -p lib.pfm --all-motifs -u -o PREFIX in.fa` end to end, from two source trees IN THE SAME JOB:
the wall time around `expect.main` (engine opened, FASTA read, every batch packed, staged and passed to the device, the files
written), with `--merge device` and `--merge host`.  The trees take turns inside every repetition; every run is a process of its
own under `timeout`, and the first one that fails ends the job.  Inputs: a generated FASTA (4096 records x 3 kb) and a library
of 8 motifs over two widths.  Medians and the spread per tree and route, and whether the trees wrote the same bytes.

    python tools/expect_driver_ab.py --trees parent=/path/to/parent,this=. [--records 4096] [--length 3000] [--widths 12,8]
                                     [--motifs 8] [--batch-records 4096] [--iters 5] [--warmup 1] [--limit 300] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from occupancy_ab import spread  # noqa: E402  (tools/ is the script's own directory)

CHILD = ("import sys, time, json\n"
         "from rnascan_amd import expect\n"
         "t0 = time.perf_counter()\n"
         "rc = expect.main(sys.argv[1:])\n"
         "print(json.dumps({'rc': rc, 'ms': (time.perf_counter() - t0) * 1e3}))\n"
         "sys.exit(rc)\n")


def write_inputs(args, directory):
    rng = np.random.default_rng(3)
    fa = os.path.join(directory, "in.fa")
    with open(fa, "w") as f:
        for r in range(args.records):
            f.write(">r%d\n%s\n" % (r, "".join(rng.choice(list("ACGU"), size=args.length))))
    widths = [int(w) for w in args.widths.split(",")]
    pfm = os.path.join(directory, "lib.pfm")
    with open(pfm, "w") as f:
        for k in range(args.motifs):
            f.write("#M%d\n#PO\tA\tC\tG\tU\n" % k)
            for j in range(widths[k % len(widths)]):
                f.write("%d\t%s\n" % (j, "\t".join("%.4f" % x for x in rng.dirichlet(np.full(4, 0.6)))))
            f.write("\n")
    return fa, pfm


def one_run(args, tree, merge, fa, pfm, prefix):
    """-> (ms around main, sha1 of the two files)"""
    env = dict(os.environ, PYTHONPATH=os.path.abspath(tree))
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, "-c", CHILD, "-p", pfm, "--all-motifs", "-u", "--merge", merge,
           "--batch-records", str(args.batch_records), "-o", prefix, fa]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, cwd=os.path.abspath(tree))
    if done.returncode != 0:
        return None, done.returncode
    digest = hashlib.sha1()
    for suffix in (".expected.txt", ".summary.txt"):
        with open(prefix + suffix, "rb") as f:
            digest.update(f.read())
    return json.loads(done.stdout.strip().splitlines()[-1])["ms"], digest.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", required=True, help="name=directory of a built source tree, comma separated; the first is the yardstick")
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--widths", default="12,8")
    ap.add_argument("--motifs", type=int, default=8)
    ap.add_argument("--batch-records", type=int, default=4096, dest="batch_records")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300, help="seconds a run may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    trees = [pair.split("=", 1) for pair in args.trees.split(",")]
    with tempfile.TemporaryDirectory() as directory:
        t0 = time.perf_counter()
        fa, pfm = write_inputs(args, directory)
        print("inputs written in %.1f s" % (time.perf_counter() - t0), flush=True)
        times = dict(((name, merge), []) for name, _ in trees for merge in ("device", "host"))
        wrote = {}
        for rep in range(args.warmup + args.iters):
            for merge in ("device", "host"):
                for name, tree in trees:
                    ms, sha = one_run(args, tree, merge, fa, pfm, os.path.join(directory, "out_%s" % name))
                    if ms is None:                                    # nothing more is started on the device after a failure
                        print("%s --merge %s ended with status %d" % (name, merge, sha), file=sys.stderr)
                        return sha
                    wrote.setdefault(sha, []).append("%s/%s" % (name, merge))
                    if rep >= args.warmup:
                        times[(name, merge)].append(ms)
                    print("rep %d %s --merge %s: %.0f ms" % (rep, name, merge, ms), flush=True)
    res = {"records": args.records, "length": args.length, "widths": args.widths, "motifs": args.motifs, "batch_records": args.batch_records,
           "same_bytes": len(wrote) == 1, "runs": dict(("%s_%s" % key, spread(ms)) for key, ms in times.items())}
    yard = trees[0][0]
    for name, _ in trees[1:]:
        for merge in ("device", "host"):
            a, b = res["runs"]["%s_%s" % (yard, merge)], res["runs"]["%s_%s" % (name, merge)]
            res["%s_%s_median_within_or_below_%s_spread" % (name, merge, yard)] = b["median_ms"] <= a["max_ms"]
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
