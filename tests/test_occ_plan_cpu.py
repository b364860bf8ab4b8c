"""The pass planner of the occupancy family (csrc/pfmscan_occ_plan.hpp) without a GPU: the header alone, compiled with
g++ -fsanitize=address,undefined beside a stand-alone driver (tests/c/occ_plan_main.cpp, its own main), against the rule
restated here, on the edge cases of the rule and on random cases, and against the invariants every driver relies on."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

FANIN, RUN = 32, 8


def plan_rule(m, n_unit, cells, wide, cap, runs, lens):
    """the rule of pfmscan_occ_plan.hpp -> (n_u_max, need_blk, need_grp, need_run, cuts, start, blk_cap, rec_cap)"""
    nb = [(max(L - m + 1, 0) + FANIN - 1) // FANIN for L in lens]
    prefix = lambda per: [sum(per[:r]) for r in range(len(per) + 1)]   # noqa: E731
    blk, grp, run = prefix(nb), prefix([(b + FANIN - 1) // FANIN for b in nb]), prefix([(b + RUN - 1) // RUN for b in nb])
    n_u_max = min(n_unit, max(1, cap // (max(max(nb, default=0), 1) * cells)))
    blk_cap, rec_cap = max(cap // (n_u_max * cells), 1), max(2 ** 30 // (n_u_max * wide), 1)
    cuts, r0 = [0], 0
    while r0 < len(lens):
        r1 = r0 + 1
        while r1 < len(lens) and r1 - r0 < rec_cap and blk[r1 + 1] - blk[r0] <= blk_cap:
            r1 += 1
        cuts.append(r1)
        r0 = r1
    need = lambda t: max((t[b] - t[a] for a, b in zip(cuts, cuts[1:])), default=0)   # noqa: E731
    return n_u_max, need(blk), need(grp), need(run) if runs else 0, cuts, blk + grp + (run if runs else []), blk_cap, rec_cap


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("occ_plan") / "occ_plan_main")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(REPO, "rnascan_amd", "csrc"), os.path.join(REPO, "tests", "c", "occ_plan_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in (m, n_unit, cells, wide, cap, runs, len(lens), *lens)) + "\n"
                       for m, n_unit, cells, wide, cap, runs, lens in cases)
        done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0 and not done.stderr, (done.stdout[-1000:] + done.stderr)[-3000:]
        plans = []
        for line in done.stdout.splitlines():
            v = [int(x) for x in line.split()]
            n_cuts = v[4]
            cuts = v[5:5 + n_cuts]
            n_start = v[5 + n_cuts]
            start = v[6 + n_cuts:]
            assert len(start) == n_start
            plans.append((v[0], v[1], v[2], v[3], cuts, start))
        assert len(plans) == len(cases)
        return plans
    return run


def check(planner, cases):
    for case, got in zip(cases, planner(cases)):
        m, n_unit, cells, wide, cap, runs, lens = case
        want = plan_rule(*case)
        assert got == want[:6], (case, got, want)
        # the invariants, directly
        n_u_max, need_blk, need_grp, need_run, cuts, start = got
        n_rec, blk_cap, rec_cap = len(lens), want[6], want[7]
        assert 1 <= n_u_max <= n_unit
        assert cuts[0] == 0 and cuts[-1] == n_rec and all(a < b for a, b in zip(cuts, cuts[1:])), (case, cuts)
        assert len(start) == (3 if runs else 2) * (n_rec + 1)
        tables = [start[i * (n_rec + 1):(i + 1) * (n_rec + 1)] for i in range(3 if runs else 2)]
        assert all(t[0] == 0 and all(a <= b for a, b in zip(t, t[1:])) for t in tables)
        for a, b in zip(cuts, cuts[1:]):
            if b - a > 1:
                assert b - a <= rec_cap and tables[0][b] - tables[0][a] <= blk_cap, (case, a, b)
        for t, need in zip(tables, (need_blk, need_grp, need_run)):
            assert need == max((t[b] - t[a] for a, b in zip(cuts, cuts[1:])), default=0)
        if not runs:
            assert need_run == 0


def test_edge_cases(planner):
    m = 5
    win = lambda w: m - 1 + w                                   # noqa: E731  a record of w windows
    sizes = [win(w) for w in (32, 33, 1024, 1025)]
    cases = []
    for cells in (1, 4, 7, 11):
        for runs in (0, 1):
            wide = 7 if cells > 1 else 1
            cases += [
                (m, 3, cells, wide, 1 << 25, runs, []),                                   # n_rec = 0
                (m, 3, cells, wide, 1 << 25, runs, [40]),                                 # n_rec = 1
                (m, 3, cells, wide, 1 << 25, runs, [0, 1, m - 1, m - 1]),                 # no record has a window
                (m, 3, cells, wide, 1 << 25, runs, [m, m - 1, m, 0, m]),                  # exactly m: one window
                (m, 3, cells, wide, 1 << 25, runs, sizes + sizes[::-1]),
                (m, 3, cells, wide, 1, runs, sizes + [m - 1, m]),                         # cap = 1: a record and a unit per pass
                (m, 20, cells, wide, 33 * cells * 20 - 1, runs, [win(1025), 40, win(1024)]),   # below the longest record's blocks: unit passes
                (m, 20, cells, wide, 33 * cells * 20, runs, [win(1025), 40, win(1024)]),       # exactly all units of the longest record
                (m, 20, cells, wide, 33 * cells - 1, runs, [win(1025), 40]),              # not even one unit fits: n_u_max = 1 all the same
                (m, 2, cells, wide, 2 * cells * 5, runs, [win(64), win(96), 40, win(33), win(1)]),      # a pass boundary met exactly (2 + 3 blocks) ...
                (m, 2, cells, wide, 2 * cells * 5 - 1, runs, [win(64), win(96), 40, win(33), win(1)]),  # ... and missed by one double
                (m, 2, cells, wide, 2 * cells * 5 + 1, runs, [win(64), win(96), 40, win(33), win(1)]),
            ]
    # n_unit * wide near 2^30 with few records: the record cap cuts, not the scratch
    for n_unit, wide in (((1 << 30) // 7, 7), ((1 << 30) // 7 + 1, 7), (1 << 30, 1), ((1 << 30) - 1, 1), ((1 << 29) + 1, 1), (1 << 29, 1), ((1 << 29) // 7, 7)):
        for cells in (1, 7, 11):
            cases.append((m, n_unit, cells, wide, 1 << 50, 1, [40, m, m - 1, 40, 40]))
            cases.append((m, n_unit, cells, wide, 1 << 50, 0, [m - 1, m - 1, m - 1]))
    check(planner, cases)


def test_random_cases(planner):
    rng = np.random.default_rng(20261020)
    cases = []
    for _ in range(4000):
        m = int(rng.integers(1, 65))
        n_rec = int(rng.integers(0, 13))
        kind = rng.integers(0, 3, size=n_rec)
        lens = np.where(kind == 0, rng.integers(0, m + 2, size=n_rec),
                        np.where(kind == 1, m - 1 + rng.choice([1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 1057], size=n_rec), rng.integers(0, 5000, size=n_rec)))
        cells = int(rng.choice([1, 4, 7, 11]))
        wide = int(rng.choice([1, 7]))
        n_unit = int(rng.choice([1, 2, 3, 17, 320, (1 << 30) // wide, (1 << 30) // wide // 3]))
        cap = int(rng.choice([1, 2, 31, 50, 157, 1000, 1 << 14, 1 << 25, 1 << 45]))
        if rng.random() < 0.3:                                      # at, or one off, what a prefix of the records needs
            nb = [(max(int(L) - m + 1, 0) + 31) // 32 for L in lens]
            cap = max(1, sum(nb[:int(rng.integers(0, n_rec + 1))]) * cells * min(n_unit, 20) + int(rng.integers(-1, 2)))
        cases.append((m, n_unit, cells, wide, cap, int(rng.integers(0, 2)), [int(v) for v in lens]))
    check(planner, cases)
