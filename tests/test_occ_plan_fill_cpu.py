"""The two optional arguments of the pass planner (csrc/pfmscan_occ_plan.hpp: ``fill_blk``, ``unit_group``), which the expected
letter-pair table of two code streams plans with, without a GPU: the header alone under g++ -fsanitize=address,undefined beside
tests/c/occ_plan_fill_main.cpp, against the rule restated here.  With both at 1 the plan is the one tests/test_occ_plan_cpu.py
holds the planner to."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from test_occ_plan_cpu import FANIN, plan_rule


def fill_rule(m, n_unit, cells, wide, cap, fill_blk, unit_group, lens):
    """-> (n_u_max, need_blk, need_grp, cuts): the units of a pass leave room for max(the longest record's blocks,
    min(fill_blk, all blocks)), rounded down to whole groups when there is more than one group's worth; the records are cut as before"""
    nb = [(max(L - m + 1, 0) + FANIN - 1) // FANIN for L in lens]
    blk = [sum(nb[:r]) for r in range(len(nb) + 1)]
    grp = [sum((b + FANIN - 1) // FANIN for b in nb[:r]) for r in range(len(nb) + 1)]
    room = max(max(nb, default=0), min(fill_blk, blk[-1]), 1)
    n_u_max = min(n_unit, max(1, cap // (room * cells)))
    if n_u_max > unit_group:
        n_u_max -= n_u_max % unit_group
    blk_cap, rec_cap = max(cap // (n_u_max * cells), 1), max(2 ** 30 // (n_u_max * wide), 1)
    cuts, r0 = [0], 0
    while r0 < len(lens):
        r1 = r0 + 1
        while r1 < len(lens) and r1 - r0 < rec_cap and blk[r1 + 1] - blk[r0] <= blk_cap:
            r1 += 1
        cuts.append(r1)
        r0 = r1
    need = lambda t: max((t[b] - t[a] for a, b in zip(cuts, cuts[1:])), default=0)   # noqa: E731
    return n_u_max, need(blk), need(grp), cuts


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("occ_plan_fill") / "occ_plan_fill_main")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(REPO, "rnascan_amd", "csrc"), os.path.join(REPO, "tests", "c", "occ_plan_fill_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in (*case[:7], len(case[7]), *case[7])) + "\n" for case in cases)
        done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0 and not done.stderr, (done.stdout[-1000:] + done.stderr)[-3000:]
        plans = []
        for line in done.stdout.splitlines():
            v = [int(x) for x in line.split()]
            plans.append((v[0], v[1], v[2], v[4:4 + v[3]]))
        assert len(plans) == len(cases)
        return plans
    return run


def test_a_library_with_the_table_gets_passes_that_fill_the_device(planner):
    """256 pairs of w = 12 with 39 scratch doubles per matrix row over 4096 records of 3 kb under the default cap: all rows in a pass
    leave room for 2 records (2048 passes of 188 blocks); planned for 16 rounds on 256 CUs a pass holds 2 whole pairs and 381 records"""
    lens = [3000] * 4096
    old, new = planner([(12, 3072, 39, 28, 1 << 25, 1, 1, lens), (12, 3072, 39, 28, 1 << 25, 16 * 256 * 8, 12, lens)])
    assert old[0] == 3072 and len(old[3]) - 1 == 2048 and old[1] == 188
    assert new[0] == 24 and len(new[3]) - 1 == 11 and new[1] == 381 * 94
    # one pair: nothing changes
    one = planner([(12, 12, 39, 28, 1 << 25, 1, 1, lens), (12, 12, 39, 28, 1 << 25, 16 * 256 * 8, 12, lens)])
    assert one[0] == one[1] and one[0][0] == 12


def test_against_the_rule(planner):
    rng = np.random.default_rng(20261021)
    cases = []
    for _ in range(3000):
        m = int(rng.integers(1, 65))
        n_rec = int(rng.integers(0, 13))
        lens = [int(v) for v in np.where(rng.random(n_rec) < 0.5, rng.integers(0, 5000, size=n_rec), m - 1 + rng.choice([0, 1, 32, 33, 1024, 1025], size=n_rec))]
        cells = int(rng.choice([28, 32, 35, 39]))
        n_unit = m * int(rng.choice([1, 2, 3, 40, 256]))
        cap = int(rng.choice([1, 50, 700, 3000, 100000, 1 << 25]))
        fill_blk = int(rng.choice([1, 2, 7, 100, 1000, 32768]))
        cases.append((m, n_unit, cells, 28, cap, fill_blk, int(rng.choice([1, m])), lens))
    for case, got in zip(cases, planner(cases)):
        assert got == fill_rule(*case), (case, got)
        m, n_unit, cells, wide, cap, fill_blk, unit_group, lens = case
        n_u_max, need_blk, _, cuts = got
        assert 1 <= n_u_max <= n_unit and (n_u_max % unit_group == 0 or n_u_max < unit_group or unit_group == 1)
        assert cuts[0] == 0 and cuts[-1] == len(lens) and all(a < b for a, b in zip(cuts, cuts[1:]))
        if fill_blk == 1 and unit_group == 1:                          # the plan of every other caller
            assert got == tuple(plan_rule(m, n_unit, cells, wide, cap, 0, lens)[i] for i in (0, 1, 2, 4))
