"""The expected letter-pair table of two code streams on a GPU-less host: the rules (tests/pair_joint_rules.py) against the three
identities of the contract and against exact rational arithmetic, the bindings of ABI 27, and ``expect_pair --joint`` with the
rules standing in for the device.  Every comparison of doubles is on bit patterns unless a bound is derived beside it."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import expect_rules as erules
import pair_joint_rules as rules
import pair_rules
from conftest import REPO
from test_occupancy_cpu import STRUCT, write_pfm
from test_pair_cpu import RNA, SEQS, STRUCTS, codes_of, outputs, run_expect, write_inputs

GOLDEN = os.path.join(REPO, "tests", "golden", "expect_pair_joint")
MODES = (rules.RATIO, rules.POSTERIOR)


# ---- the rules -------------------------------------------------------------------------------------------------------
def test_the_margins_that_come_with_the_table_are_the_pair_rules():
    rng = np.random.default_rng(3)
    for m in (1, 5):
        codes, codes2, off, lens = rules.streams(rng, [0, m - 1, m, m + 40, 1100][::-1], foreign_seq=0.03, foreign_struct=0.03, case=True)
        R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
        for mode in MODES:
            es, et, ej, occ, win = rules.expected(codes, codes2, off, lens, R, S, mode)
            e2, t2, o2, w2 = pair_rules.expected(codes, codes2, off, lens, R, S, mode)
            assert rules.same_bits(es, e2) and rules.same_bits(et, t2) and rules.same_bits(occ, o2) and np.array_equal(win, w2)
            assert ej.shape == (lens.size, 1, m, 4, 8) and (ej[..., 7] == 0).all() and not np.signbit(ej).any()


@pytest.mark.parametrize("mode", MODES)
def test_identities_1_and_2_a_constant_stream(mode):
    rng = np.random.default_rng(60 + mode)
    m = 8
    lengths = [int(x) + m - 1 for x in rng.integers(1, 200, size=10)] + [m - 1, 1024 + m - 1, 1100 + m]
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.01)
    b0 = rng.integers(0, 7, size=lens.size)
    for r in range(lens.size):
        codes2[off[r]:off[r] + lens[r]] = np.uint8(b0[r] | (8 if r % 2 else 0))
    es, et, ej, occ, win = rules.expected(codes, codes2, off, lens, R, S, mode)
    for r in range(lens.size):
        assert rules.same_bits(ej[r, 0, :, :, b0[r]], es[r, 0, :, :4]) and (np.delete(ej[r, 0], b0[r], axis=2) == 0).all()
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_struct=0.01, case=True)
    a0 = rng.integers(0, 4, size=lens.size)
    for r in range(lens.size):
        codes[off[r]:off[r] + lens[r]] = np.uint8(a0[r])
    es, et, ej, occ, win = rules.expected(codes, codes2, off, lens, R, S, mode)
    for r in range(lens.size):
        assert rules.same_bits(ej[r, 0, :, a0[r], :], et[r, 0]) and (np.delete(ej[r, 0], a0[r], axis=1) == 0).all()
    assert (occ > 0).any()


def test_identity_3_tables_of_ones_count_letter_pairs():
    rng = np.random.default_rng(8)
    for m in (1, 8):
        codes, codes2, off, lens = rules.streams(rng, list(range(0, 70)) + [1500], case=True)
        es, et, ej, occ, win = rules.expected(codes, codes2, off, lens, rules.ones(m), rules.ones(m), rules.RATIO)
        J = rules.pair_counts(codes, codes2, off, lens, m)
        assert not J[:, 4:].any() and not J[:, :, 7].any() and int(J.sum()) == m * int(np.maximum(lens - m + 1, 0).sum())
        assert np.array_equal(ej[:, 0].sum(axis=0), J[:, :4].astype(np.float64))
        assert np.array_equal(occ[:, 0], np.maximum(lens - m + 1, 0)) and np.array_equal(win, np.maximum(lens - m + 1, 0))


@pytest.mark.parametrize("mode", MODES)
def test_the_table_sums_to_the_margins_exactly_before_rounding(mode):
    """m = 3, 40 windows: over the same weights in exact rational arithmetic the rows of the table add up to E_seq and its
    columns to E_struct, and every cell of the rules is within the tree's bound of its exact sum (terms >= 0)"""
    rng = np.random.default_rng(70 + mode)
    m, n_win = 3, 40
    codes, codes2, off, lens = rules.streams(rng, [n_win + m - 1], foreign_seq=0.03, foreign_struct=0.03)
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    es, et, ej, occ, win = rules.expected_record(codes, codes2, 0, lens[0], R, S, mode)
    e2, t2, _, _ = pair_rules.expected(codes, codes2, off, lens, R, S, mode)
    assert rules.same_bits(es, e2[0, 0]) and rules.same_bits(et, t2[0, 0]) and 0 < win < n_win
    t, has = pair_rules.terms(codes, codes2, 0, lens[0], R, S)
    w = [Fraction(float(x)) for x in erules.weights(t, has, occ, mode)]
    a, b = codes & 7, codes2 & 7
    bound = Fraction(erules.tree_bound(n_win))
    for k in range(m):
        J = [[sum((w[s] for s in range(n_win) if has[s] and a[s + k] == ca and b[s + k] == cb), Fraction(0)) for cb in range(7)] for ca in range(4)]
        for ca in range(4):
            exact = sum((w[s] for s in range(n_win) if has[s] and a[s + k] == ca), Fraction(0))
            assert sum(J[ca], Fraction(0)) == exact and abs(Fraction(float(es[k, ca])) - exact) <= bound * exact
        for cb in range(7):
            exact = sum((w[s] for s in range(n_win) if has[s] and b[s + k] == cb), Fraction(0))
            assert sum((J[ca][cb] for ca in range(4)), Fraction(0)) == exact and abs(Fraction(float(et[k, cb])) - exact) <= bound * exact
        for ca in range(4):
            for cb in range(7):
                assert abs(Fraction(float(ej[k, ca, cb])) - J[ca][cb]) <= bound * J[ca][cb]


# ---- bindings --------------------------------------------------------------------------------------------------------
def test_abi_27_exports_the_joint_entry_points():
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == L.pfmscan_abi_version() == 27
    for name in ("pfmscan_expect_pair_joint_dev", "pfmscan_expect_pair_joint_staged", "pfmscan_expect_pair_joint_merged_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
    for name in ("expect_pair_joint_dev", "expect_pair_joint_staged", "expect_pair_joint_merged_staged"):
        assert callable(getattr(_lib.Context, name))
    assert callable(scanner.HipEngine.expect_pair_joint) and callable(scanner.HipEngine.expect_pair_joint_merged)


# ---- the command with the rules in the device's place ------------------------------------------------------------------
class _RuleEngine(object):
    """HipEngine.expect_pair / expect_pair_joint answered by the rules; ``calls`` names what the command asked for"""

    def __init__(self, spoil=None):
        self.calls, self.spoil = [], spoil

    def expect_pair(self, stream, seq_tables, struct_tables, mode):
        self.calls.append("expect_pair")
        return pair_rules.expected(stream.codes, stream.codes2, stream.offsets, stream.lengths, seq_tables, struct_tables, mode)

    def expect_pair_joint(self, stream, seq_tables, struct_tables, mode):
        self.calls.append("expect_pair_joint")
        got = rules.expected(stream.codes, stream.codes2, stream.offsets, stream.lengths, seq_tables, struct_tables, mode)
        if self.spoil is not None:
            self.spoil(stream, got[2])
        return got

    def close(self):
        pass


def joint_rows(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def pfms(tmp_path, widths=(6, 4)):
    return write_pfm(tmp_path / "seq.pfm", RNA, widths, seed=3), write_pfm(tmp_path / "st.pfm", STRUCT, widths, seed=4)


def test_joint_file_columns_cells_and_mutual_information(tmp_path):
    from rnascan_amd import expect, expect_pair, fasta, pssm, sites
    fa, sfa = write_inputs(tmp_path)
    seq, st = pfms(tmp_path)
    sodds, todds = pssm.load_odds(seq, 0.02, fasta.RNA, None), pssm.load_odds(st, 0.02, fasta.STRUCT, None)
    for weight in ("posterior", "ratio"):
        base = ["-p", seq, "-q", st, "-u", "-C", "0.02", "--struct-format", "letters", "--weight", weight, "--joint"]
        engine = _RuleEngine()
        assert run_expect(engine, base + ["--all-motifs", "-o", str(tmp_path / weight), fa, sfa]) == 0
        assert set(engine.calls) == {"expect_pair_joint"}
        header, rows = joint_rows(str(tmp_path / weight) + ".expected.joint.txt")
        assert header == ["Motif", "PO"] + ["%s.%s" % (a, b) for a in "ACGU" for b in "BEHLMRT"] + ["MI"] == ["Motif", "PO"] + sites.JOINT_NAMES + ["MI"]
        assert [r[:2] for r in rows] == [["M0", str(k)] for k in range(6)] + [["M1", str(k)] for k in range(4)]     # pair order
        at = 0
        for mid, m in (("M0", 6), ("M1", 4)):
            per = [rules.expected_record(codes_of(s, RNA), codes_of(t, STRUCT), 0, len(s), sodds[mid].ratio_table(RNA),
                                         todds[mid].ratio_table(STRUCT), expect.MODES[weight]) for (_, s), t in zip(SEQS, STRUCTS)]
            for k in range(m):
                cells = [[math.fsum(p[2][k, a, STRUCT.index(b)] for p in per) for b in "BEHLMRT"] for a in range(4)]
                assert rows[at][2:30] == [repr(c) for row in cells for c in row]
                assert [float(x) for x in rows[at][2:30]] == [c for row in cells for c in row]            # reads back to the same double
                total = math.fsum(c for row in cells for c in row)
                pa, pb = [math.fsum(row) / total for row in cells], [math.fsum(row[b] for row in cells) / total for b in range(7)]
                mi = math.fsum((c / total) * math.log2((c / total) / (pa[a] * pb[b])) for a, row in enumerate(cells) for b, c in enumerate(row) if c)
                assert rows[at][30] == repr(mi) and mi > 0 and expect_pair.mutual_information(cells) == mi
                at += 1
        # the first pair alone: no Motif column, the same numbers
        assert run_expect(_RuleEngine(), base + ["-o", str(tmp_path / "one"), fa, sfa]) == 0
        h1, r1 = joint_rows(str(tmp_path / "one") + ".expected.joint.txt")
        assert h1 == header[1:] and r1 == [r[1:] for r in rows[:6]]
    assert expect_pair.mutual_information([[0.0] * 7] * 4) == 0.0
    ints = [[3, 0, 1, 0, 0, 2, 0], [0, 4, 0, 0, 1, 0, 0], [1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 5, 0, 0, 2]]
    assert expect_pair.mutual_information([[float(c) for c in row] for row in ints]) == sites.mutual_information(ints)


def test_without_joint_nothing_changes(tmp_path):
    """the three files have the bytes they had before the option existed (tests/golden/expect_pair_joint, written by the
    command at the commit before it, on these inputs and the rules), no joint file appears and the table is never asked for"""
    fa, sfa = write_inputs(tmp_path)
    seq, st = pfms(tmp_path)
    for name, extra in (("library", ["--all-motifs"]), ("two", ["--iterations", "2"])):
        engine = _RuleEngine()
        argv = ["-p", seq, "-q", st, "-u", "-C", "0.02", "--struct-format", "letters"] + extra + ["-o", str(tmp_path / name), fa, sfa]
        assert run_expect(engine, argv) == 0
        assert set(engine.calls) == {"expect_pair"} and not os.path.exists(str(tmp_path / name) + ".expected.joint.txt")
        for suffix, text in zip((".expected.seq.txt", ".expected.struct.txt", ".summary.txt"), outputs(tmp_path / name)):
            assert text == open(os.path.join(GOLDEN, name + suffix)).read(), (name, suffix)
        # with --joint: the same three files, and the fourth
        assert run_expect(_RuleEngine(), argv[:-2] + ["--joint"] + argv[-2:]) == 0
        assert outputs(tmp_path / name) == tuple(open(os.path.join(GOLDEN, name + s)).read() for s in (".expected.seq.txt", ".expected.struct.txt", ".summary.txt"))
        assert os.path.exists(str(tmp_path / name) + ".expected.joint.txt")


def joint_outputs(prefix):
    return outputs(prefix) + (open(str(prefix) + ".expected.joint.txt").read(),)


def test_iterations_batches_and_record_order(tmp_path):
    fa, sfa = write_inputs(tmp_path)
    seq, st = pfms(tmp_path)
    base = ["-C", "0.02", "--struct-format", "letters", "--all-motifs", "--joint"]
    # --iterations 2 --joint is a run on the outputs of a run, byte for byte: the table is the last pass's, the margins are fed back
    assert run_expect(_RuleEngine(), ["-p", seq, "-q", st] + base + ["--iterations", "2", "-o", str(tmp_path / "two"), fa, sfa]) == 0
    assert run_expect(_RuleEngine(), ["-p", seq, "-q", st] + base + ["-o", str(tmp_path / "first"), fa, sfa]) == 0
    assert run_expect(_RuleEngine(), ["-p", str(tmp_path / "first") + ".expected.seq.txt", "-q", str(tmp_path / "first") + ".expected.struct.txt"] +
                      base + ["-o", str(tmp_path / "second"), fa, sfa]) == 0
    two, first, second = joint_outputs(tmp_path / "two"), joint_outputs(tmp_path / "first"), joint_outputs(tmp_path / "second")
    assert two[:2] == second[:2] and two[3] == second[3] and two[3] != first[3]
    # --batch-records 1 and a shuffled record order write the same bytes
    assert run_expect(_RuleEngine(), ["-p", seq, "-q", st] + base + ["--batch-records", "1", "-o", str(tmp_path / "b1"), fa, sfa]) == 0
    assert joint_outputs(tmp_path / "b1") == first
    order = [3, 0, 4, 2, 1]
    (tmp_path / "shuffled").mkdir()
    sfa2, fa2 = tmp_path / "shuffled" / "structs.fa", tmp_path / "shuffled" / "seqs.fa"
    fa2.write_text("".join(">%s\n%s\n" % SEQS[i] for i in order))
    sfa2.write_text("".join(">%s\n%s\n" % (SEQS[i][0], STRUCTS[i]) for i in order))
    assert run_expect(_RuleEngine(), ["-p", seq, "-q", st] + base + ["--batch-records", "2", "-o", str(tmp_path / "sh"), str(fa2), str(sfa2)]) == 0
    assert joint_outputs(tmp_path / "sh") == first


def test_a_nan_that_only_the_table_holds_is_the_runs_failure(tmp_path, capsys):
    """the table goes through the same non-finite check as the two matrices, after them: exit 1, the pair and the record named"""
    fa, sfa = write_inputs(tmp_path)
    seq, st = pfms(tmp_path, (6, 6))                                     # one width: both pairs in one call

    def spoil(stream, ej):
        ej[3, 1, 2, 1, 4] = np.nan                                       # record r4, pair M1
    prefix = str(tmp_path / "out")
    argv = ["-p", seq, "-q", st, "-u", "-C", "0.02", "--struct-format", "letters", "--all-motifs", "--joint", "-o", prefix, fa, sfa]
    assert run_expect(_RuleEngine(spoil), argv) == 1
    err = capsys.readouterr().err
    assert "Motif M1" in err and "record r4" in err and "M0" not in err and ("infinite" in err or "not a number" in err)
    assert not any(os.path.exists(prefix + s) for s in (".expected.seq.txt", ".expected.struct.txt", ".expected.joint.txt", ".summary.txt"))


def read_pfm_rows(path, n_letters):
    rows = [ln.split("\t") for ln in open(path).read().splitlines() if ln and not ln.startswith("#") and not ln.startswith("PO")]
    return [[float(x) for x in r[1:1 + n_letters]] for r in rows]


def test_written_table_against_the_written_margins(tmp_path):
    """|sum_b J[k][a][b] - E_seq[k][a]| <= 2 (N + 40) 2^-53 E_seq[k][a], N the longest record's windows, the sum over b exact
    (fractions): every term is >= 0, so each tree sum carries at most that relative error (at most N - 1 rounded additions on a
    path is a generous count for the tree) and the record sums are exact; the same for the columns against E_struct"""
    fa, sfa = write_inputs(tmp_path)
    seq, st = pfms(tmp_path, (6,))
    prefix = str(tmp_path / "out")
    assert run_expect(_RuleEngine(), ["-p", seq, "-q", st, "-u", "-C", "0.02", "--struct-format", "letters", "--joint", "-o", prefix, fa, sfa]) == 0
    _, rows = joint_rows(prefix + ".expected.joint.txt")
    J = np.asarray([[float(x) for x in r[1:29]] for r in rows]).reshape(6, 4, 7)
    Es, Et = read_pfm_rows(prefix + ".expected.seq.txt", 4), read_pfm_rows(prefix + ".expected.struct.txt", 7)
    N = max(len(s) for _, s in SEQS) - 6 + 1
    bound = Fraction(2 * (N + 40)) * Fraction(2) ** -53
    seen = 0
    for k in range(6):
        for a in range(4):
            exact = sum((Fraction(float(x)) for x in J[k, a]), Fraction(0))
            assert abs(exact - Fraction(Es[k][a])) <= bound * Fraction(Es[k][a])
            seen += Es[k][a] > 0
        for b in range(7):
            exact = sum((Fraction(float(x)) for x in J[k, :, b]), Fraction(0))
            assert abs(exact - Fraction(Et[k][b])) <= bound * Fraction(Et[k][b])
    assert seen > 12
