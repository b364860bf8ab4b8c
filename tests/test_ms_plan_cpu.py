"""The pass plan of the multi-site model (csrc/pfmscan_ms_plan.hpp) without a GPU: the header alone, compiled with g++
-fsanitize=address,undefined beside a stand-alone driver (tests/c/ms_plan_main.cpp, its own main), against what a plan must
satisfy: every (record, motif) lies in exactly one pass, in order; a pass's planes hold its records' positions; two planes of a
pass stay inside the cap unless the pass is one record under one motif; `need` is the largest pass."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("ms_plan") / "ms_plan_main")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(REPO, "rnascan_amd", "csrc"), os.path.join(REPO, "tests", "c", "ms_plan_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in (cap, n_mo, len(recs), *[x for r in recs for x in r])) + "\n" for cap, n_mo, recs in cases)
        done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0 and not done.stderr, (done.stdout[-1000:] + done.stderr)[-3000:]
        got = []
        for line in done.stdout.splitlines():
            v = [int(x) for x in line.split()]
            assert len(v[2:]) == 6 * v[1]
            got.append((v[0], [tuple(v[2 + 6 * i:8 + 6 * i]) for i in range(v[1])]))
        assert len(got) == len(cases)
        return got
    return run


def check(plan, cases):
    for (cap, n_mo, recs), (need, passes) in zip(cases, plan(cases)):
        seen, biggest = [], 0
        for r0, r1, q0, nq, base, span in passes:
            assert 0 <= r0 < r1 <= len(recs) and 0 <= q0 and nq >= 1 and q0 + nq <= n_mo
            assert base == recs[r0][0] and span == recs[r1 - 1][0] + recs[r1 - 1][1] - base
            for o, n in recs[r0:r1]:
                assert base <= o and o + n <= base + span
            assert 2 * span * nq <= max(cap, 2) or (r1 - r0 == 1 and nq == 1)
            seen += [(r, q) for r in range(r0, r1) for q in range(q0, q0 + nq)]
            biggest = max(biggest, 2 * span * nq)
        assert sorted(seen) == [(r, q) for r in range(len(recs)) for q in range(n_mo)] and len(set(seen)) == len(seen)
        # records ascend from pass to pass, motifs within a record range
        assert [(p[0], p[2]) for p in passes] == sorted((p[0], p[2]) for p in passes)
        assert need == biggest


def table(rng, n_rec, hi, gap=2):
    lens = rng.integers(0, hi, size=n_rec)
    off, recs = int(rng.integers(0, 5)), []
    for n in lens:
        recs.append((off, int(n)))
        off += int(n) + int(rng.integers(0, gap + 1))
    return recs


def test_edge_cases(plan):
    rng = np.random.default_rng(1)
    cases = [(100, 3, []), (100, 0, [(0, 5)]), (1, 2, [(0, 0), (0, 0)]), (2, 1, [(0, 1), (1, 1)]), (1, 3, [(3, 7), (10, 0), (12, 5)]),
             (2 ** 62, 5, table(rng, 9, 50)), (10 ** 6, 64, [(0, 3 * 10 ** 9)]), (16, 4, [(0, 4), (4, 4), (8, 4), (100, 4)])]
    check(plan, cases)
    # all records and all motifs in one pass when the cap allows it
    got = plan([(2 ** 40, 7, [(0, 10), (11, 20), (40, 0)])])[0]
    assert got == (2 * 40 * 7, [(0, 3, 0, 7, 0, 40)])


def test_random_cases(plan):
    rng = np.random.default_rng(20261021)
    cases = []
    for _ in range(2000):
        recs = table(rng, int(rng.integers(0, 14)), int(rng.choice([3, 40, 700])), gap=int(rng.choice([0, 1, 50])))
        total = sum(n for _, n in recs) + 1
        cases.append((int(rng.choice([1, 2, 7, total // 2 + 1, total, 2 * total, 5 * total, 40 * total])), int(rng.integers(1, 6)), recs))
    check(plan, cases)
