"""The tile prefix of the posterior site map on profiles (csrc/pfmscan_fp_plan.hpp) without a GPU: the header alone, compiled
with g++ -fsanitize=address,undefined beside a stand-alone driver (tests/c/fp_plan_main.cpp, its own main), against the rule
restated here: ceil(L / tile) tiles per record numbered in record order, and -1 once the call passes 2^31 - 1 tiles."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

MAX_TILES = 2 ** 31 - 1


def prefix_rule(tile, lens):
    """-> (n_tiles or -1, the prefix as far as it was made, zeros behind)"""
    out = [0] * (len(lens) + 1)
    for r, L in enumerate(lens):
        n = -(-L // tile)
        if out[r] + n > MAX_TILES:
            return -1, out
        out[r + 1] = out[r] + n
    return out[-1], out


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("fp_plan") / "fp_plan_main")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(REPO, "rnascan_amd", "csrc"), os.path.join(REPO, "tests", "c", "fp_plan_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in (tile, len(lens), *lens)) + "\n" for tile, lens in cases)
        done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0 and not done.stderr, (done.stdout[-1000:] + done.stderr)[-3000:]
        got = []
        for line in done.stdout.splitlines():
            v = [int(x) for x in line.split()]
            assert len(v[2:]) == v[1]
            got.append((v[0], v[2:]))
        assert len(got) == len(cases)
        return got
    return run


def check(prefix, cases):
    for case, got in zip(cases, prefix(cases)):
        assert got == prefix_rule(*case), (case, got)


def test_edge_cases(prefix):
    big = 2 ** 63 - 1
    cases = []
    for tile in (1, 193, 245, 256, 449, 512):                       # SLOTS - (m - 1) for m = 64, 12, 1 at 256 and 512 slots; and 1
        cases += [(tile, []), (tile, [0]), (tile, [0, 0, 0]), (tile, [1]), (tile, [tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1]),
                  (tile, [5, 0, 3 * tile + 7, 0, 1]),
                  (tile, [MAX_TILES * tile]),                       # exactly the limit
                  (tile, [MAX_TILES * tile + 1]),                   # one tile over: -1
                  (tile, [(MAX_TILES - 1) * tile, 1]), (tile, [(MAX_TILES - 1) * tile, 1, 1]), (tile, [(MAX_TILES - 1) * tile, 0, tile + 1, 9]),
                  (tile, [big]), (tile, [big, big]), (tile, [3, big, 7])]   # lengths near 2^63: no sum overflows
    check(prefix, cases)


def test_random_cases(prefix):
    rng = np.random.default_rng(20261021)
    cases = []
    for _ in range(3000):
        m = int(rng.integers(1, 65))
        tile = int(rng.choice([256, 512])) - (m - 1)
        n_rec = int(rng.integers(0, 13))
        kind = rng.integers(0, 3, size=n_rec)
        lens = np.where(kind == 0, rng.integers(0, m + 2, size=n_rec),
                        np.where(kind == 1, rng.choice([tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 1], size=n_rec) + rng.choice([0, m - 1], size=n_rec),
                                 rng.integers(0, 5000, size=n_rec)))
        lens = [int(v) for v in lens]
        if lens and rng.random() < 0.1:                              # around the limit of a launch
            lens[int(rng.integers(0, n_rec))] = (MAX_TILES - int(rng.integers(0, 40))) * tile + int(rng.integers(-1, 2))
        cases.append((tile, lens))
    check(prefix, cases)
