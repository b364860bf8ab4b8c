"""Occupancy on a GPU-less host: pssm.odds against pssm.log_odds, the rules (tests/occupancy_rules.py) against independent
arithmetic, the bindings, and the command's host logic with the rules standing in for the device."""
import io
import math
import os
import re

import numpy as np
import pytest

import occupancy_rules as rules
from conftest import DATA_DIR, REPO

RNA, STRUCT = "ACGU", "EHTBLRM"          # code order of the streams (pack.RNA_LETTERS, pack.STRUCT_LETTERS)


def ulps(a, b):
    """distance in units of the last place of finite doubles of one sign pattern ordering"""
    def key(x):
        i = np.asarray(x, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(key(a) - key(b))


def check_odds_against_log_odds(pwm, background):
    from rnascan_amd import pssm
    lo, od = pssm.log_odds(pwm, background), pssm.odds(pwm, background)
    assert list(lo.keys()) == list(od.keys())
    for l in lo:
        cell, R = lo[l], od[l]
        assert R.dtype == np.float64 and R.shape == cell.shape
        assert not np.signbit(R[~np.isnan(R)]).any()                       # never negative, never -0.0
        assert np.array_equal(np.isnan(R), np.isnan(cell))                  # NaN <-> NaN
        assert np.array_equal(R == 0, np.isneginf(cell))                    # 0 <-> -inf
        assert np.array_equal(np.isposinf(R), np.isposinf(cell))            # inf <-> +inf
        fin = np.isfinite(cell)
        assert np.isfinite(R[fin]).all() and (R[fin] > 0).all()
        if fin.any():
            assert ulps(np.log2(R[fin]), cell[fin]).max() <= 2


def random_pwm(rng, m, letters, zeros=0.0):
    from collections import OrderedDict
    from rnascan_amd import pssm
    M = rng.dirichlet(np.full(len(letters), 0.5), size=m) * rng.integers(1, 500)
    M[rng.random(M.shape) < zeros] = 0.0
    return OrderedDict((l, M[:, k].copy()) for k, l in enumerate(letters)), pssm


@pytest.mark.parametrize("letters", ["GAUC", STRUCT])
def test_odds_is_log_odds_before_the_log(letters):
    rng = np.random.default_rng(len(letters))
    for trial in range(40):
        counts, pssm = random_pwm(rng, int(rng.integers(1, 30)), letters, zeros=0.2 if trial % 2 else 0.0)
        for pc in (0.0, 0.01, 1.0):
            pwm = pssm.normalize(counts, pc)
            check_odds_against_log_odds(pwm, None)
            bg = dict((l, float(x)) for l, x in zip(letters, rng.random(len(letters)) + 0.01))
            check_odds_against_log_odds(pwm, bg)
            bg[letters[trial % len(letters)]] = 0.0                          # b == 0: +inf where p > 0, NaN where p == 0
            check_odds_against_log_odds(pwm, bg)


@pytest.mark.parametrize("name,letters", [("test_seq_pfm.txt", "GAUC"), ("SLBP_pfm_assembled_normalized_seq.txt", "GAUC"),
                                          ("test_struct_pfm.txt", STRUCT), ("SLBP_pfm_assembled_normalized_struct.txt", STRUCT)])
def test_odds_on_the_shipped_pfms(name, letters):
    from collections import OrderedDict
    from rnascan_amd import pssm
    path = os.path.join(DATA_DIR, name)
    counts = pssm.read_pfm(path)
    counts = OrderedDict((l, counts[l]) for l in letters)
    bg = dict((l, 0.05 + 0.1 * k) for k, l in enumerate(letters))
    for pc in (0.0, 0.01):
        for b in (None, bg):
            check_odds_against_log_odds(pssm.normalize(counts, pc), b)
            od = pssm.load_odds(path, pc, letters, b)
            lo = pssm.load_pssms(path, pc, letters, b)
            assert list(od.keys()) == list(lo.keys())
            code = RNA if letters == "GAUC" else STRUCT
            for mid in od:
                R = od[mid].ratio_table(code)
                assert R.shape == (lo[mid].length, 8) and np.isnan(R[:, len(code):]).all()
                # the rules' own table from the same counts: the same bits
                # (normalised in the alphabet's letter order, as pssm.normalize does, then put into code order)
                C = np.stack([counts[l] for l in letters], axis=1)
                by_letter = rules.ratio_table(C, None if b is None else [b[l] for l in letters], pc)
                want = np.full_like(by_letter, np.nan)
                for k, l in enumerate(letters):
                    want[:, code.index(l)] = by_letter[:, k]
                assert rules.same_bits(R, want)


def test_rules_ratio_table_special_cells():
    R = rules.ratio_table([[1, 0, 3, 0], [2, 2, 0, 0]], [0.5, 0.5, 0.0, 0.0])
    assert R[0, 0] == 0.5 and R[0, 1] == 0 and not np.signbit(R[0, 1]) and np.isposinf(R[0, 2]) and np.isnan(R[0, 3])
    assert np.isnan(R[:, 4:]).all()


def test_term_is_two_to_the_score():
    """log2(term) against the exact sum (math.fsum) of the window's PSSM cells, bound from the rules file"""
    from collections import OrderedDict
    from rnascan_amd import pssm
    rng = np.random.default_rng(5)
    for m in (1, 2, 8, 12, 21, 64):
        counts = OrderedDict((l, rng.random(m) + 0.05) for l in "GAUC")
        pwm = pssm.normalize(counts, 0.01)
        bg = dict(zip("GAUC", [0.3, 0.2, 0.26, 0.24]))
        T = pssm.PSSM("GAUC", pssm.log_odds(pwm, bg)).letter_table(RNA)
        R = pssm.Odds("GAUC", pssm.odds(pwm, bg)).ratio_table(RNA)
        codes, off, lens = rules.stream(rng, [400])
        t, has = rules.terms(codes, off[0], lens[0], R, 4)
        assert has.all() and (t > 0).all() and np.isfinite(t).all()
        for s in range(t.size):
            cells = [T[k, codes[s + k]] for k in range(m)]
            assert abs(math.log2(t[s]) - math.fsum(cells)) <= rules.term_log2_bound(m, cells)


@pytest.mark.parametrize("n_win", [1, 2, 31, 32, 33, 1023, 1024, 1025, 32768, 32769])
def test_tree_against_fsum(n_win):
    rng = np.random.default_rng(n_win)
    t = np.exp(rng.uniform(-20, 20, size=n_win))
    got, want = rules.tree(t), math.fsum(t.tolist())
    assert abs(got - want) <= rules.tree_bound(n_win) * want
    assert rules.depth(n_win) == (0 if n_win == 1 else 1 if n_win <= 32 else 2 if n_win <= 1024 else 3 if n_win <= 32768 else 4)


def test_tree_is_the_definition_on_a_small_case():
    """33 terms: element 0 of level 1 is ((t0 + t1) + ...) + t31, element 1 is t32; level 2 their sum"""
    t = np.ldexp(1.0, -np.arange(33) * 3).astype(np.float64) * 1.1
    s = t[0]
    for x in t[1:32]:
        s = s + x
    assert rules.tree(t) == s + t[32]
    assert rules.tree(np.zeros(0)) == 0.0 and not np.signbit(rules.tree(np.zeros(0)))


def test_terms_skip_foreign_windows_and_ignore_case():
    rng = np.random.default_rng(2)
    R = rules.table(rng, 3, 7)
    codes = np.array([0, 1 | 8, 2, 7, 3, 4, 5, 6 | 8, 7], dtype=np.uint8)
    t, has = rules.terms(codes, 0, 8, R, 7)
    assert has.tolist() == [True, False, False, False, True, True]
    assert t[0] == R[0, 0] * R[1, 1] * R[2, 2] and t[1] == 0 and t[5] == R[0, 4] * R[1, 5] * R[2, 6]
    t4, has4 = rules.terms(codes, 0, 8, R, 4)                               # the same bytes as RNA: codes 4..7 are foreign
    assert has4.tolist() == [True, False, False, False, False, False]
    occ, win = rules.occupancy(codes, [0], [8], R, 7)
    assert win[0] == 3 and occ[0, 0] == (t[0] + 0.0 + 0.0 + 0.0 + t[4]) + t[5]


# ---- bindings --------------------------------------------------------------------------------------------------------
def test_abi_21_exports_the_occupancy_entry_points():
    from rnascan_amd import _lib, build
    build.build_lib()
    L = _lib.load()
    assert _lib.ABI_VERSION >= 21 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) >= 21
    assert int(re.search(r"#define\s+PFMSCAN_OCC_FANIN\s+(\d+)", text).group(1)) == _lib.OCC_FANIN == rules.FANIN
    for name in ("pfmscan_occupancy_dev", "pfmscan_occupancy_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
    assert "pfmscan_occupancy.hip" in build.SOURCES


# ---- the command with the rules in the device's place ------------------------------------------------------------------
class _RuleEngine(object):
    """HipEngine.occupancy answered by the rules"""

    def occupancy(self, stream, ratio_tables, n_letters, which=0):
        return rules.occupancy(stream.codes2 if which else stream.codes, stream.offsets, stream.lengths, ratio_tables, n_letters)

    def close(self):
        pass


FASTA = ">r1 first\nACGUACGUAAGGCUCUUUUCAGAGCACGU\n>r2\nacgtnacgtAAAGGCTCTTTTCAGAGCAA\n>r3\nGG\n>r4\n" + "ACGGU" * 30 + "\n"


def write_pfm(path, letters, widths, seed=0, zero=False):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for k, m in enumerate(widths):
            if len(widths) > 1:
                f.write("#M%d\n#" % k)
            f.write("PO\t" + "\t".join(letters) + "\n")
            for j in range(m):
                row = rng.dirichlet(np.full(len(letters), 0.4))
                if zero and j == 1:
                    row[0] = 0.0
                f.write("%d\t%s\n" % (j, "\t".join("%.4f" % x for x in row)))
            f.write("\n")
    return str(path)


def run_command(engine, argv):
    from rnascan_amd import occupancy
    out = io.StringIO()
    rc = occupancy.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def test_command_rows_and_batching(tmp_path):
    from rnascan_amd import occupancy, pssm
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    pfm = write_pfm(tmp_path / "m.pfm", "ACGU", (6, 4, 6), seed=3, zero=True)
    base = ["-p", pfm, "-u", "-C", "0", "--all-motifs"]
    rc, text = run_command(_RuleEngine(), base + [str(fa)])
    assert rc == 0
    lines = text.splitlines()
    assert lines[0].split("\t") == occupancy.COLUMNS and len(lines) == 1 + 4 * 3
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [r[1] for r in rows] == ["r1"] * 3 + ["r2"] * 3 + ["r3"] * 3 + ["r4"] * 3         # record order, then the file's motif order
    assert [r[0] for r in rows[:3]] == ["M0", "M1", "M2"]
    assert rows[6][2:] == ["0", "0.0", "-inf"] and rows[7][2:] == ["0", "0.0", "-inf"]        # r3 is shorter than every motif
    r1, r2 = FASTA.split("\n")[1], FASTA.split("\n")[3]
    assert rows[0][2] == str(len(r1) - 5) and rows[1][2] == str(len(r1) - 3)
    assert r2[4] == "n" and rows[3][2] == str(len(r2) - 5 - 5)                                # the windows over the n have no term
    odds = pssm.load_odds(pfm, 0.0, "GAUC", None)
    for r in rows:
        x = float(r[3])
        assert repr(x) == r[3]                                                                 # the shortest string that round-trips
        assert r[4] == ("-inf" if x == 0 else repr(round(math.log2(x), 3)))
    codes = np.array(["ACGU".index(c) for c in "ACGUACGUAAGGCUCUUUUCAGAGCACGU"], dtype=np.uint8)
    want, _ = rules.occupancy(np.append(codes, 7), [0], [codes.size], odds["M1"].ratio_table(RNA), 4)
    assert float(rows[1][3]) == want[0, 0]
    for n in ("1", "3"):
        assert run_command(_RuleEngine(), base + ["--batch-records", n, str(fa)])[1] == text
    first = run_command(_RuleEngine(), ["-p", pfm, "-u", str(fa)])[1].splitlines()
    assert first[1:] == [ln for ln in lines[1:] if ln.startswith("M0\t")]                     # without --all-motifs: the first motif


def test_command_log2_column():
    from rnascan_amd import occupancy
    assert occupancy.log2_text(0.0) == "-inf" and occupancy.log2_text(math.inf) == "inf" and occupancy.log2_text(math.nan) == "nan"
    assert occupancy.log2_text(8.0) == "3.0" and occupancy.log2_text(5e-324) == "-1074.0" and occupancy.log2_text(3.0) == "1.585"


def test_command_argument_errors(tmp_path, capsys):
    """exit 1 and a message that names the option, before any device is opened"""
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (5,))
    wide = write_pfm(tmp_path / "wide.pfm", "ACGU", (65,))
    wide_q = write_pfm(tmp_path / "wideq.pfm", STRUCT, (70,))
    for argv, needles in ((["-p", seq, "-q", st, str(fa)], ("-p", "-q")), ([str(fa)], ("-p", "-q")),
                          (["-p", wide, "-u", str(fa)], ("-p", "PFMSCAN_MAX_M", "65")), (["-q", wide_q, "-u", str(fa)], ("-q", "PFMSCAN_MAX_M"))):
        rc, text = run_command(None, argv)
        err = capsys.readouterr().err
        assert rc == 1 and text == ""
        for needle in needles:
            assert needle in err
