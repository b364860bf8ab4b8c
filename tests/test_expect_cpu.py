"""Expected counts on a GPU-less host: the rules (tests/expect_rules.py) against their identities and derived bounds, the
bindings, and the command's host logic with the rules standing in for the device."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import expect_rules as rules
import occupancy_rules as orules
from conftest import REPO
from test_gpu_occupancy import length_ladder
from test_occupancy_cpu import STRUCT, write_pfm

RNA = "ACGU"


# ---- the rules -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladders():
    """the length ladder once per (m, n_letters): the stream, the table and the rules' answer in both modes"""
    cache = {}

    def get(m, nl):
        if (m, nl) not in cache:
            rng = np.random.default_rng(1000 + 10 * m + nl)
            codes, off, lens = orules.stream(rng, length_ladder(rng, m), nl, foreign=0.002, case=nl == 7)
            R = orules.table(rng, m, nl, 0.5, 2.0)
            cache[(m, nl)] = (codes, off, lens, R, dict((mode, rules.expected(codes, off, lens, R, nl, mode)) for mode in (rules.RATIO, rules.POSTERIOR)))
        return cache[(m, nl)]
    return get


@pytest.mark.parametrize("m,nl", [(12, 4), (64, 4), (21, 7)])
def test_identities_and_bounds_on_the_ladder(ladders, m, nl):
    codes, off, lens, R, want = ladders(m, nl)
    n_win = np.maximum(lens - m + 1, 0)
    for n in (0, 1, 31, 32, 33, 1023, 1024, 1025, 32768, 32769):
        assert (n_win == n).any()
    occ_want = orules.occupancy(codes, off, lens, R, nl)
    for mode in (rules.RATIO, rules.POSTERIOR):
        exp, occ, win = want[mode]
        assert exp.shape == (lens.size, 1, m, 8)
        assert orules.same_bits(occ, occ_want[0]) and np.array_equal(win, occ_want[1])      # the occupancy's own bits and Windows
        assert (exp[:, :, :, nl:] == 0).all() and not np.signbit(exp).any() and np.isfinite(exp).all()
        assert (exp[n_win == 0] == 0).all()
        for r in range(lens.size):
            o = float(occ[r, 0])
            if win[r] == 0:
                assert o == 0 and (exp[r] == 0).all()
                continue
            sums = rules.column_sums(exp[r, 0], nl)
            if mode == rules.RATIO:
                bound = Fraction(rules.ratio_column_bound(int(n_win[r]))) * Fraction(o)
                assert all(abs(s - Fraction(o)) <= bound for s in sums)
            else:
                bound = Fraction(rules.posterior_column_bound(int(n_win[r])))
                assert all(abs(s - 1) <= bound for s in sums)


def test_a_lone_window_is_copied():
    rng = np.random.default_rng(3)
    R = orules.table(rng, 5, 4)
    codes = np.array([2, 0, 3, 3, 1, 7], dtype=np.uint8)
    t = R[0, 2] * R[1, 0] * R[2, 3] * R[3, 3] * R[4, 1]
    E, occ, win = rules.expected_record(codes, 0, 5, R, 4, rules.RATIO)
    assert occ == t and win == 1
    want = np.zeros((5, 8))
    for k, c in enumerate(codes[:5]):
        want[k, c] = t
    assert orules.same_bits(E, want)
    E, occ, win = rules.expected_record(codes, 0, 5, R, 4, rules.POSTERIOR)
    assert orules.same_bits(E, np.where(want > 0, t * (1.0 / t), 0.0))


def test_tree_rows_is_the_occupancy_tree_row_by_row():
    rng = np.random.default_rng(4)
    for n in (1, 2, 31, 32, 33, 1025, 40000):
        X = np.exp(rng.uniform(-20, 20, size=(5, n))) * (rng.random((5, n)) < 0.4)
        assert orules.same_bits(rules.tree_rows(X), [orules.tree(row) for row in X])
    assert orules.same_bits(rules.tree_rows(np.zeros((3, 0))), np.zeros(3))


@pytest.mark.parametrize("nl", [4, 7])
def test_uniform_table_in_ratio_mode_counts_letters(nl):
    """every ratio is 1.0: E is the integer count of every letter under every column over the windows with a term"""
    rng = np.random.default_rng(nl)
    m = 9
    codes, off, lens = orules.stream(rng, [3, 8, 9, 40, 700, 5000], nl, foreign=0.02, case=nl == 7)
    R = np.full((m, 8), np.nan)
    R[:, :nl] = 1.0
    exp, occ, win = rules.expected(codes, off, lens, R, nl, rules.RATIO)
    for r, (o, n) in enumerate(zip(off, lens)):
        c = codes[o:o + n] & 7
        want = np.zeros((m, 8))
        for s in range(max(n - m + 1, 0)):
            if (c[s:s + m] < nl).all():
                for k in range(m):
                    want[k, c[s + k]] += 1
        assert np.array_equal(exp[r, 0], want) and occ[r, 0] == win[r] == want[0].sum()


def test_zero_occupancy_and_special_cells():
    rng = np.random.default_rng(6)
    m = 4
    codes, off, lens = orules.stream(rng, [60], 4)
    R = orules.table(rng, m, 4)
    R[1, :4] = 0.0                                                       # every term is +0.0: occ is +0.0
    for mode in (rules.RATIO, rules.POSTERIOR):
        E, occ, win = rules.expected_record(codes, off[0], lens[0], R, 4, mode)
        assert occ == 0 and win == 57 and (E == 0).all() and not np.signbit(E).any()
    R = orules.table(rng, m, 4)
    R[2, 1] = np.inf
    E, occ, _ = rules.expected_record(codes, off[0], lens[0], R, 4, rules.POSTERIOR)
    assert np.isposinf(occ) and np.isnan(E[:, :4]).any()                 # v = 1 / inf = 0, and inf * 0 is NaN: IEEE as it falls
    E, occ, _ = rules.expected_record(codes, off[0], lens[0], R, 4, rules.RATIO)
    assert np.isposinf(E[2, 1]) and np.isfinite(E[2, 0])


# ---- bindings --------------------------------------------------------------------------------------------------------
def test_abi_23_exports_the_expect_entry_points():
    from rnascan_amd import _lib, build
    build.build_lib()
    L = _lib.load()
    assert _lib.ABI_VERSION >= 23 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) >= 23
    assert int(re.search(r"#define\s+PFMSCAN_EXPECT_RATIO\s+(\d+)", text).group(1)) == _lib.EXPECT_RATIO == rules.RATIO
    assert int(re.search(r"#define\s+PFMSCAN_EXPECT_POSTERIOR\s+(\d+)", text).group(1)) == _lib.EXPECT_POSTERIOR == rules.POSTERIOR
    for name in ("pfmscan_expect_dev", "pfmscan_expect_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
    assert "pfmscan_expect.hip" in build.SOURCES
    assert callable(_lib.Context.expect_dev) and callable(_lib.Context.expect_staged)
    from rnascan_amd import scanner
    assert callable(scanner.HipEngine.expect)


# ---- the command with the rules in the device's place ------------------------------------------------------------------
class _RuleEngine(object):
    """HipEngine.expect answered by the rules"""

    def expect(self, stream, ratio_tables, n_letters, mode, which=0):
        return rules.expected(stream.codes2 if which else stream.codes, stream.offsets, stream.lengths, ratio_tables, n_letters, mode)

    def close(self):
        pass


FASTA = ">r1 first\nACGUACGUAAGGCUCUUUUCAGAGCACGU\n>r2\nacgtnacgtAAAGGCTCTTTTCAGAGCAA\n>r3\nGG\n>r4\n" + "ACGGU" * 30 + "\n>r5\nNNNNNNNNNNNN\n"
STRUCT_FASTA = ">s1\nEEEHHHHLLLLHHHHTTT\n>s2\nEEhhhllllhhhTTeemmmBBBrrr\n>s3\nEHHHHHHHHLLLLLLRRRRMMMMBBBBBTTT\n"


def run_command(engine, argv):
    from rnascan_amd import expect
    return expect.main(argv, engine=engine)


def outputs(prefix):
    with open(str(prefix) + ".expected.txt") as f, open(str(prefix) + ".summary.txt") as g:
        return f.read(), g.read()


def test_command_columns_and_first_motif(tmp_path):
    from rnascan_amd import expect, pssm
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    pfm = write_pfm(tmp_path / "m.pfm", RNA, (6,), seed=3)
    for weight in ("posterior", "ratio"):
        assert run_command(_RuleEngine(), ["-p", pfm, "-u", "-C", "0.01", "--weight", weight, "-o", str(tmp_path / weight), str(fa)]) == 0
        pfm_text, summary = outputs(tmp_path / weight)
        lines = summary.splitlines()
        assert lines[0].split("\t") == expect.COLUMNS and len(lines) == 2
        row = lines[1].split("\t")
        # r3 is shorter than the motif and r5 holds no window with a term: skipped; r2's windows over the n have no term
        assert row[:5] == ["m", "1", "3", "2", str((29 - 5) + (29 - 5 - 5) + (150 - 5))]
        # the written file is a PFM that reads back to the rules' sums, the records added exactly
        got = pssm.read_pfm(str(tmp_path / weight) + ".expected.txt")
        assert list(got.keys()) == list(RNA) and all(v.size == 6 for v in got.values())
        R = pssm.load_odds(pfm, 0.01, "GAUC", None)["m"].ratio_table(RNA)
        per, occ = [], []
        for body in [ln for ln in FASTA.splitlines() if not ln.startswith(">")]:
            codes = np.array([RNA.index(c) if c in RNA else 7 for c in body.upper().replace("T", "U")] + [7], dtype=np.uint8)
            E, o, _ = rules.expected_record(codes, 0, codes.size - 1, R, 4, expect.MODES[weight])
            per.append(E)
            occ.append(o)
        for c, l in enumerate(RNA):
            assert got[l].tolist() == [math.fsum(E[k, c] for E in per) for k in range(6)]
        assert row[5] == repr(round(math.fsum(math.log2(o) for o in occ if o > 0), 3))
        if weight == "posterior":
            assert all(abs(sum(got[l][k] for l in RNA) - 3) < 1e-12 for k in range(6))     # one site per counted record


def test_command_motif_order_over_two_widths_and_batching(tmp_path):
    from rnascan_amd import pssm
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    pfm = write_pfm(tmp_path / "lib.pfm", RNA, (6, 4, 6), seed=5)
    base = ["-p", pfm, "-C", "0.1", "--all-motifs"]
    assert run_command(_RuleEngine(), base + ["-o", str(tmp_path / "a"), str(fa)]) == 0
    text, summary = outputs(tmp_path / "a")
    assert [ln.split("\t")[0] for ln in summary.splitlines()[1:]] == ["M0", "M1", "M2"]
    lib = list(pssm.read_multi_pfm(str(tmp_path / "a") + ".expected.txt"))
    assert [mid for mid, _ in lib] == ["M0", "M1", "M2"] and [c["A"].size for _, c in lib] == [6, 4, 6]
    for n in ("1", "2", "3"):
        assert run_command(_RuleEngine(), base + ["--batch-records", n, "-o", str(tmp_path / ("b" + n)), str(fa)]) == 0
        assert outputs(tmp_path / ("b" + n)) == (text, summary)
    # without --all-motifs: the first motif, as a single PFM; its numbers are the library's first block
    assert run_command(_RuleEngine(), ["-p", pfm, "-C", "0.1", "-o", str(tmp_path / "one"), str(fa)]) == 0
    one, one_summary = outputs(tmp_path / "one")
    assert not one.startswith("#") and [ln.split("\t")[0] for ln in one_summary.splitlines()[1:]] == ["M0"]
    assert one.splitlines()[1:] == text.splitlines()[2:8]
    # the records in another order: exact sums do not depend on it
    blocks = FASTA.strip().split("\n>")
    (tmp_path / "rev.fa").write_text(">" + "\n>".join(b.lstrip(">") for b in reversed(blocks)) + "\n")
    assert run_command(_RuleEngine(), base + ["-u", "-o", str(tmp_path / "fwd"), str(fa)]) == 0
    assert run_command(_RuleEngine(), base + ["-u", "-o", str(tmp_path / "rev"), str(tmp_path / "rev.fa")]) == 0
    assert outputs(tmp_path / "fwd") == outputs(tmp_path / "rev")


@pytest.mark.parametrize("kind", ["seq", "struct"])
def test_two_iterations_are_two_chained_runs(tmp_path, kind):
    if kind == "seq":
        fa, option, letters, widths = FASTA, "-p", RNA, (6, 4)
    else:
        fa, option, letters, widths = STRUCT_FASTA, "-q", STRUCT, (5, 3)
    (tmp_path / "in.fa").write_text(fa)
    src = str(tmp_path / "in.fa")
    for extra, w in ((["--all-motifs"], widths), ([], widths[:1])):
        pfm = write_pfm(tmp_path / ("m%d.pfm" % len(w)), letters, w, seed=7)
        base = ["-C", "0.02", "--struct-format", "letters"] + extra
        assert run_command(_RuleEngine(), [option, pfm] + base + ["--iterations", "2", "-o", str(tmp_path / "two"), src]) == 0
        assert run_command(_RuleEngine(), [option, pfm] + base + ["-o", str(tmp_path / "first"), src]) == 0
        assert run_command(_RuleEngine(), [option, str(tmp_path / "first") + ".expected.txt"] + base + ["-o", str(tmp_path / "second"), src]) == 0
        two, two_summary = outputs(tmp_path / "two")
        first, first_summary = outputs(tmp_path / "first")
        second, second_summary = outputs(tmp_path / "second")
        assert two == second and two != first
        rows = [ln.split("\t") for ln in two_summary.splitlines()[1:]]
        assert [r[1] for r in rows] == ["1"] * len(w) + ["2"] * len(w)                       # one line per motif and iteration
        assert [r[2:] for r in rows[:len(w)]] == [ln.split("\t")[2:] for ln in first_summary.splitlines()[1:]]
        assert [r[2:] for r in rows[len(w):]] == [ln.split("\t")[2:] for ln in second_summary.splitlines()[1:]]


def test_lower_case_structure_letters_count_as_their_letter(tmp_path):
    (tmp_path / "mixed.fa").write_text(STRUCT_FASTA)
    (tmp_path / "upper.fa").write_text("".join(ln if ln.startswith(">") else ln.upper() for ln in STRUCT_FASTA.splitlines(True)))
    pfm = write_pfm(tmp_path / "st.pfm", STRUCT, (5,), seed=9)
    for name in ("mixed", "upper"):
        assert run_command(_RuleEngine(), ["-q", pfm, "-u", "-C", "0.05", "--struct-format", "letters", "-o", str(tmp_path / name), str(tmp_path / (name + ".fa"))]) == 0
    assert outputs(tmp_path / "mixed") == outputs(tmp_path / "upper")
    header = outputs(tmp_path / "mixed")[0].splitlines()[0].split("\t")
    assert header == ["PO"] + list("BEHLMRT")                             # the column order of the shipped structure PFMs


def test_errors_before_a_device_is_opened(tmp_path, capsys):
    """exit 1, a message that names the cause, nothing written, and no engine asked for"""
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (5,))
    wide = write_pfm(tmp_path / "wide.pfm", RNA, (65,))
    avg = tmp_path / "avgdir"
    avg.mkdir()
    prefix = str(tmp_path / "out")
    for argv, needles in ((["-p", seq, "-q", st, str(fa)], ("-p", "-q")), ([str(fa)], ("-p", "-q")),
                          (["-p", wide, "-u", str(fa)], ("-p", "PFMSCAN_MAX_M", "65")),
                          (["-p", seq, "--iterations", "0", str(fa)], ("--iterations",)),
                          (["-q", st, str(avg)], ("averaged-structure", "not supported"))):
        rc = run_command(None, ["-o", prefix] + argv)
        err = capsys.readouterr().err
        assert rc == 1
        for needle in needles:
            assert needle in err
        assert not os.path.exists(prefix + ".expected.txt") and not os.path.exists(prefix + ".summary.txt")


def test_errors_after_the_pass(tmp_path, capsys):
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    prefix = str(tmp_path / "out")
    # a background of 0 for a letter the motif has: a ratio is +inf, r1's occupancy with it
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    bg = tmp_path / "bg.txt"
    bg.write_text("{'A': 0.0, 'C': 0.3, 'G': 0.3, 'U': 0.4}")
    assert run_command(_RuleEngine(), ["-p", seq, "-C", "0.01", "-b", str(bg), "-o", prefix, str(fa)]) == 1
    err = capsys.readouterr().err
    assert "Motif seq" in err and "record r1" in err and ("infinite" in err or "not a number" in err)
    # a motif no record contributes to: every window of every record meets a zero
    with open(str(tmp_path / "zero.pfm"), "w") as f:
        f.write("PO\tA\tC\tG\tU\n0\t1\t1\t1\t1\n1\t0\t0\t0\t0\n")
    assert run_command(_RuleEngine(), ["-p", str(tmp_path / "zero.pfm"), "-u", "-o", prefix, str(fa)]) == 1
    err = capsys.readouterr().err
    assert "Motif zero" in err and "no record contributes" in err
    assert not os.path.exists(prefix + ".expected.txt") and not os.path.exists(prefix + ".summary.txt")
