"""The expected nucleotide x context table on averaged-structure profiles on a GPU-less host: the rules
(tests/expect_profile_joint_rules.py) against the three identities of the contract, against deliberate mistakes and against a
derived bound on the margins; the bindings; and ``expect_profile --joint`` with the rules standing in for the device.  Every
comparison of doubles is on bit patterns unless a bound is derived beside it."""
import math
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

import expect_merge_rules as mrules
import expect_profile_joint_rules as rules
import expect_profile_rules as xrules
import expect_rules as erules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import pair_joint_rules as jrules
import test_expect_profile_cpu as pcpu
from conftest import REPO
from test_occupancy_profile_cpu import DATA_DIR, FILE_ORDER, STRUCT, make_inputs, write_pfm

MODES = (rules.RATIO, rules.POSTERIOR)
LADDER = [0, 1, 2, 31, 32, 33, 255, 256, 257, 1024, 1025]             # windows


def ladder(m):
    return [n + m - 1 for n in LADDER]


# ---- the rules: the three identities -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", MODES)
def test_identity_1_a_constant_nucleotide(mode, dtype):
    rng = np.random.default_rng(11 + mode)
    for m in (1, 8, 12):
        codes, profile, off, lens = prules.stream(rng, ladder(m), dtype)
        a0 = rng.integers(0, 4, size=lens.size)
        for r in range(lens.size):
            codes[off[r]:off[r] + lens[r]] = np.uint8(a0[r] | (8 if r % 2 else 0))          # bit 3 (lower case) is not the letter
        R, S = orules.table(rng, m), prules.struct_table(rng, m)
        for st in (S, None):
            es, eq, ej, occ, win = rules.expected(profile, codes, off, lens, R, st, mode)
            for r in range(lens.size):
                assert rules.same_bits(ej[r, 0, :, a0[r], :], es[r, 0])
                assert (np.delete(ej[r, 0], a0[r], axis=1) == 0).all() and not np.signbit(np.delete(ej[r, 0], a0[r], axis=1)).any()
            assert (occ[2:] > 0).all() and (ej[..., 7] == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", MODES)
def test_identity_2_one_hot_rows_are_the_letter_pair_table(mode, dtype):
    """finite positive tables, identity column order: w * 1.0 is w, w * 0.0 is +0.0, and the marginal of a one-hot row is the
    table's cell, so the table is pair_joint_rules' table of the letters argmax(row), which selects where this one multiplies"""
    rng = np.random.default_rng(21 + mode)
    for m in (1, 8, 12):
        letters, off, lens = orules.stream(rng, ladder(m), 7, case=False)
        codes, _, _, _ = prules.stream(rng, ladder(m), dtype, foreign=0.01)
        profile = prules.one_hot(letters, dtype)
        letters = letters.copy()
        letters[letters > 6] = 7                                                            # separators stay foreign
        R, S = orules.table(rng, m), prules.struct_table(rng, m)
        S8 = np.full((m, 8), np.nan)
        S8[:, :7] = S
        es, eq, ej, occ, win = rules.expected(profile, codes, off, lens, R, S, mode)
        for r in range(lens.size):
            qs, qt, qj, qo, qw = jrules.expected_record(codes, letters, off[r], lens[r], R, S8, mode)
            assert rules.same_bits(ej[r, 0], qj) and rules.same_bits(es[r, 0], qt) and rules.same_bits(eq[r, 0], qs)
            assert rules.same_bits(occ[r, 0], qo) and win[r] == qw
        assert (ej[3:] > 0).any(axis=(1, 2, 3, 4)).all()


def nucleotide_counts(codes, off, lens, m):
    """int64 [n_rec][m][4]: the windows of a record under whose column k nucleotide a lies"""
    out = np.zeros((len(off), m, 4), dtype=np.int64)
    for r, (o, n) in enumerate(zip(off, lens)):
        n_win = max(int(n) - m + 1, 0)
        c = np.asarray(codes[int(o):int(o) + int(n)]).astype(np.int64) & 7
        for k in range(m):
            out[r, k] = np.bincount(c[k:k + n_win], minlength=4)[:4]
    return out


DYADIC_ROW = np.array([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.015625])     # sums to 1.0 in any order of addition


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_3_tables_of_ones_count_nucleotides(dtype):
    """R and S all 1.0, ratio weights, no foreign code.  With the letter chain alone every weight is 1.0 and rows of seven 0.5 give
    0.5 x the count.  In the joint chain the marginal of such a row is 3.5, not 1.0: the weight is 3.5^m, and the table
    3.5^m x 0.5 x the count -- exact while it fits 53 bits, which it does here.  Rows of dyadic cells that sum to 1.0 have the
    marginal 1.0: the table is the cell x the count"""
    rng = np.random.default_rng(31)
    for m in (1, 8):
        codes, profile, off, lens = prules.stream(rng, ladder(m), dtype)
        counts = nucleotide_counts(codes, off, lens, m).astype(np.float64)
        R, S = np.ones((m, 8)), np.ones((m, 7))
        profile[:] = 0.5
        es, eq, ej, occ, win = rules.expected(profile, codes, off, lens, R, None, rules.RATIO)
        assert np.array_equal(ej[:, 0, :, :, :7], 0.5 * counts[:, :, :, None] * np.ones(7)) and np.array_equal(eq[:, 0, :, :4], counts)
        es, eq, ej, occ, win = rules.expected(profile, codes, off, lens, R, S, rules.RATIO)
        assert np.array_equal(ej[:, 0, :, :, :7], 3.5 ** m * 0.5 * counts[:, :, :, None] * np.ones(7)) and 3.5 ** m * 0.5 * counts.max() < 2.0 ** 53
        profile[:] = DYADIC_ROW.astype(dtype)
        es, eq, ej, occ, win = rules.expected(profile, codes, off, lens, R, S, rules.RATIO)
        assert np.array_equal(ej[:, 0, :, :, :7], counts[:, :, :, None] * DYADIC_ROW) and np.array_equal(occ[:, 0], np.maximum(lens - m + 1, 0))
        assert counts.sum() == m * np.maximum(lens - m + 1, 0).sum()


# ---- the deliberate mistakes ---------------------------------------------------------------------------------------------
def _fused(profile, codes, off, length, R, S, mode):
    """the table of one record if s + w * r were contracted: the product exact, one rounding after the addition (an FMA).  The
    first value of a block is a product rounded on its own; levels 1 and up have no products"""
    t, has = prules.terms(profile, off, length, S, codes, R)
    w = erules.weights(t, has, orules.tree(t), mode)
    x = np.asarray(profile[int(off):int(off) + int(length)]).astype(np.float64)
    cd = np.asarray(codes[int(off):int(off) + int(length)]) & 7
    m, n_win = R.shape[0], t.size
    E = np.zeros((m, 4, 8))
    for k in range(m):
        for a in range(4):
            for c in range(7):
                sums = []
                for b0 in range(0, n_win, 32):
                    s = None
                    for i in range(b0, min(b0 + 32, n_win)):
                        on = has[i] and cd[i + k] == a
                        if s is None:
                            s = float(w[i] * x[i + k, c]) if on else 0.0
                        elif on:
                            s = float(Fraction(s) + Fraction(float(w[i])) * Fraction(float(x[i + k, c])))
                    sums.append(s)
                E[k, a, c] = orules.tree(np.asarray(sums)) if len(sums) > 1 else sums[0]
    return E


def _unpadded(X):
    """expect_rules.tree_rows that adds the children that exist instead of padding every level with +0.0"""
    a = np.asarray(X, dtype=np.float64)
    while a.shape[1] > 1:
        full = a.shape[1] // 32 * 32
        parts = []
        if full:
            b = a[:, :full].reshape(a.shape[0], -1, 32)
            s = b[:, :, 0]
            for i in range(1, 32):
                s = s + b[:, :, i]
            parts.append(s)
        if a.shape[1] > full:
            s = a[:, full]
            for i in range(full + 1, a.shape[1]):
                s = s + a[:, i]
            parts.append(s[:, None])
        a = np.concatenate(parts, axis=1)
    return a[:, 0].copy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_deliberate_mistakes_give_other_bits(dtype):
    rng = np.random.default_rng(41)
    m = 3
    codes, profile, off, lens = prules.stream(rng, [70 + m - 1, 33 + m - 1], dtype)
    R, S = orules.table(rng, m), prules.struct_table(rng, m)
    for mode in MODES:
        right = rules.expected(profile, codes, off, lens, R, S, mode)[2]
        assert np.isfinite(right).all() and (right[:, 0, :, :, :7] > 0).all()
        # the select dropped: every nucleotide gets exp_struct
        dropped = rules.expected(profile, codes, off, lens, R, S, mode, sel=lambda has, ck, a: has)[2]
        assert (dropped.view(np.uint64) != right.view(np.uint64))[:, 0, :, :, :7].all()
        # the product fused into the addition: the same quantity, other bits
        fused = np.stack([_fused(profile, codes, o, n, R, S, mode) for o, n in zip(off, lens)])
        assert (fused.view(np.uint64) != right[:, 0].view(np.uint64)).any(axis=(1, 2, 3)).all() and np.allclose(fused, right[:, 0], rtol=1e-12)
    # the padding omitted: a column of -0.0 under 33 windows is +0.0 by the rules (the +0.0 of the padding) and -0.0 without it;
    # under 32 windows and under a lone one nothing is padded and it stays -0.0
    codes, profile, off, lens = prules.stream(rng, [33 + m - 1, 32 + m - 1, m], dtype)
    codes[:] &= 3
    codes[off[0]:off[0] + lens[0]] = 2
    codes[off[1]:off[1] + lens[1]] = 1
    codes[off[2]:off[2] + lens[2]] = 0
    profile[:, 3] = -0.0
    good = rules.expected(profile, codes, off, lens, R, S, rules.RATIO)[2]
    bad = rules.expected(profile, codes, off, lens, R, S, rules.RATIO, tree_rows=_unpadded)[2]
    assert not np.signbit(good[0, 0, :, 2, 3]).any() and np.signbit(bad[0, 0, :, 2, 3]).all()
    assert np.signbit(good[1, 0, :, 1, 3]).all() and np.signbit(good[2, 0, :, 0, 3]).all()
    assert rules.same_bits(np.delete(good, 3, axis=4), np.delete(bad, 3, axis=4)) and rules.same_bits(good[1:], bad[1:])


# ---- the margins, to a derived bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", MODES)
def test_the_table_sums_to_exp_struct_within_the_trees_bound(mode, dtype):
    """rules.margin_bound: the sum over the nucleotides, taken exactly, against exp_struct; the bound from the tree's depth and
    the exact sum of |x_s|.  Foreign codes are in: their windows have no term in either"""
    rng = np.random.default_rng(51 + mode)
    m = 4
    codes, profile, off, lens = prules.stream(rng, [1, 33, 257, 1025, 1500], dtype, foreign=0.005)
    lens = lens.copy()
    R, S = orules.table(rng, m), prules.struct_table(rng, m)
    checked = 0
    for st in (S, None):
        es, eq, ej, occ, win = rules.expected(profile, codes, off, lens, R, st, mode)
        for r in range(lens.size):
            n_win = max(int(lens[r]) - m + 1, 0)
            if n_win == 0:
                continue
            t, has = prules.terms(profile, off[r], lens[r], st, codes, R) if st is not None else orules.terms(codes, off[r], lens[r], R, 4)
            w = erules.weights(t, has, orules.tree(t), mode)
            x = np.asarray(profile[int(off[r]):int(off[r]) + int(lens[r])]).astype(np.float64)
            for k in range(m):
                for c in range(7):
                    vals = np.where(has, w * x[k:k + n_win, c], 0.0)
                    A = sum((Fraction(abs(float(v))) for v in vals), Fraction(0))
                    total = sum((Fraction(float(v)) for v in ej[r, 0, k, :, c]), Fraction(0))
                    assert abs(total - Fraction(float(es[r, 0, k, c]))) <= rules.margin_bound(n_win, A)
                    checked += 1
    assert checked == 2 * 4 * m * 7 and rules.margin_bound(1, Fraction(1)) == 0 and rules.tree_depth(1025) == 3


# ---- bindings ----------------------------------------------------------------------------------------------------------------
def _c_arguments(text, name):
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_the_header_and_the_bindings_declare_the_same_entry_points():
    import ctypes
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == L.pfmscan_abi_version() == 27
    added = {"_dev": ["double *d_exp_joint"], "_staged": ["double *exp_joint"], "_merged_staged": ["uint64_t *acc_joint", "int64_t *bad_joint"]}
    for suffix, more in added.items():
        name, base = "pfmscan_expect_profile_joint" + suffix, "pfmscan_expect_profile" + suffix
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
        args, old = _c_arguments(text, name), _c_arguments(text, base)
        assert [a for a in args if a not in more] == old and [a for a in args if a in more] == more     # the namesake's list plus the table
        types = getattr(L, name).argtypes
        assert len(types) == len(args)
        for a, t in zip(args, types):
            want = ctypes.c_int32 if a.startswith("int ") else ctypes.c_int64 if a.startswith("int64_t ") and "*" not in a else ctypes.c_void_p
            assert t is want, (name, a)
    for name in ("expect_profile_joint_dev", "expect_profile_joint_staged", "expect_profile_joint_merged_staged"):
        assert callable(getattr(_lib.Context, name))
    assert callable(scanner.HipEngine.expect_profile_joint) and callable(scanner.HipEngine.expect_profile_joint_merged)


# ---- the command with the rules in the device's place ----------------------------------------------------------------------
class _RuleEngine(pcpu._RuleEngine):
    """HipEngine.expect_profile_joint answered by the rules; ``names`` lists what the command asked for"""

    def __init__(self, spoil=None):
        pcpu._RuleEngine.__init__(self)
        self.names, self.spoil = [], spoil

    def expect_profile(self, stream, struct_tables, seq_tables, mode):
        self.names.append("expect_profile")
        return pcpu._RuleEngine.expect_profile(self, stream, struct_tables, seq_tables, mode)

    def expect_profile_joint(self, stream, struct_tables, seq_tables, mode):
        self.names.append("expect_profile_joint")
        got = rules.expected(stream.profile, stream.codes, stream.offsets, stream.lengths, seq_tables, struct_tables, mode)
        if self.spoil is not None:
            self.spoil(stream, got)
        return got


class _MergedEngine(_RuleEngine):
    def expect_profile_joint_merged(self, stream, struct_tables, seq_tables, mode, acc_struct, acc_seq, acc_joint):
        from test_expect_merge_cpu import merge_into
        es, eq, ej, o, w = self.expect_profile_joint(stream, struct_tables, seq_tables, mode)
        return merge_into(acc_struct, es), merge_into(acc_seq, eq), merge_into(acc_joint, ej.reshape(ej.shape[:2] + (-1, 8))), o, w

    def expect_profile_merged(self, stream, struct_tables, seq_tables, mode, acc_struct, acc_seq=None):
        from test_expect_merge_cpu import merge_into
        es, eq, o, w = self.expect_profile(stream, struct_tables, seq_tables, mode)
        return merge_into(acc_struct, es), (None if acc_seq is None else merge_into(acc_seq, eq)), o, w


def joint_rows(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def joint_outputs(prefix):
    return pcpu.outputs(prefix) + (open(str(prefix) + ".expected.joint.txt").read(),)


def rule_tables(data, ids, struct_odds, seq_odds, mode, orders=None):
    """the table of the records ``ids`` by the rules, each record in ITS stored column order, mapped to FILE_ORDER and added
    exactly -> [m][4][7], the last axis in FILE_ORDER (the written order)"""
    per = []
    for sid in ids:
        seq, rows = data[sid]
        cols = orders[int(sid[1:])] if orders else FILE_ORDER
        profile = np.ascontiguousarray(rows[:, [STRUCT.index(c) for c in cols]])
        S = None if struct_odds is None else np.stack([struct_odds[c] for c in cols], axis=1)
        codes = np.array(["ACGU".index(c) if c in "ACGU" else 7 for c in seq], dtype=np.uint8)
        ej = rules.joint_record(profile, codes, 0, len(seq), seq_odds.ratio_table("ACGU"), S, mode)
        per.append(ej[:, :, [cols.index(c) for c in FILE_ORDER]])
    return np.array([[[math.fsum(e[k, a, c] for e in per) for c in range(7)] for a in range(4)] for k in range(per[0].shape[0])])


@pytest.mark.parametrize("weight", ["posterior", "ratio"])
def test_joint_file_columns_cells_and_mutual_information(tmp_path, weight):
    from rnascan_amd import expect, expect_pair, pssm, sites
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4), seed=2, ids=["A", "B"])
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=3, ids=["A", "B"])
    s_odds, q_odds = pssm.load_odds(stp, 0.01, "EHTBLRM", None), pssm.load_odds(seq, 0.01, "GAUC", None)
    assert list(FILE_ORDER) == list(sites.STRUCT_ORDER)
    for form, opts in (("joint", ["-p", seq, "-q", stp]), ("seq", ["-p", seq])):
        base = opts + ["-u", "-C", "0.01", "--weight", weight, "--joint"]
        engine = _RuleEngine()
        prefix = str(tmp_path / form)
        assert pcpu.run_command(engine, base + ["--all-motifs", "-o", prefix, fa, d]) == 0
        assert set(engine.names) == {"expect_profile_joint"}
        header, rows = joint_rows(prefix + ".expected.joint.txt")
        assert header == ["Motif", "PO"] + ["%s.%s" % (a, b) for a in "ACGU" for b in "BEHLMRT"] + ["MI"] == ["Motif", "PO"] + sites.JOINT_NAMES + ["MI"]
        assert [r[:2] for r in rows] == [["A", str(k)] for k in range(6)] + [["B", str(k)] for k in range(4)]
        at = 0
        for mid, m in (("A", 6), ("B", 4)):
            J = rule_tables(data, sorted(data), s_odds[mid] if form == "joint" else None, q_odds[mid], expect.MODES[weight])
            for k in range(m):
                cells = J[k].tolist()
                assert rows[at][2:30] == [repr(c) for row in cells for c in row]
                assert rows[at][30] == repr(expect_pair.mutual_information(cells)) and float(rows[at][30]) > 0
                at += 1
        # the first motif (pair) alone: no Motif column, the same numbers; batches, the store and the record order change no byte
        one = str(tmp_path / "one")
        assert pcpu.run_command(_RuleEngine(), base + ["-o", one, fa, d]) == 0
        h1, r1 = joint_rows(one + ".expected.joint.txt")
        assert h1 == header[1:] and r1 == [r[1:] for r in rows[:6]]
        want = joint_outputs(prefix)
        for extra, source in ((["--batch-records", "1"], d), (["--batch-records", "4"], st)):
            assert pcpu.run_command(_RuleEngine(), base + ["--all-motifs"] + extra + ["-o", one, fa, source]) == 0
            assert joint_outputs(one) == want
        # without --joint: the same other files, no joint file, the table never asked for
        engine = _RuleEngine()
        plain = str(tmp_path / "plain")
        assert pcpu.run_command(engine, [o for o in base if o != "--joint"] + ["--all-motifs", "-o", plain, fa, d]) == 0
        assert set(engine.names) == {"expect_profile"} and pcpu.outputs(plain) == want[:3] and not os.path.exists(plain + ".expected.joint.txt")


def test_two_column_orders_and_two_iterations(tmp_path):
    from rnascan_amd import pssm
    other = "EHTBLRM"
    orders = [FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER]
    fa, mixed, _, data, order = make_inputs(tmp_path, orders=orders, name="mixed")
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.0, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.0, "GAUC", None).values()))
    base = ["-p", seq, "-q", stp, "-u", "--joint"]
    m_ = str(tmp_path / "m")
    assert pcpu.run_command(_RuleEngine(), base + ["-o", m_, fa, mixed]) == 0
    _, rows = joint_rows(m_ + ".expected.joint.txt")
    J = rule_tables(data, sorted(data), s_odds, q_odds, rules.POSTERIOR, orders)
    assert [r[1:29] for r in rows] == [[repr(c) for row in J[k].tolist() for c in row] for k in range(6)]
    for n in ("1", "2"):
        assert pcpu.run_command(_RuleEngine(), base + ["--batch-records", n, "-o", str(tmp_path / "b"), fa, mixed]) == 0
        assert joint_outputs(tmp_path / "b") == joint_outputs(m_)
    # --iterations 2 is a run on the outputs of a run: the table is the last pass's and is not fed back
    (tmp_path / "it").mkdir()
    fa, d, st, data, order = make_inputs(tmp_path / "it")
    base = ["-C", "0.02", "--joint"]
    first, second, two = str(tmp_path / "first"), str(tmp_path / "second"), str(tmp_path / "two")
    assert pcpu.run_command(_RuleEngine(), ["-p", seq, "-q", stp] + base + ["--iterations", "2", "-o", two, fa, st]) == 0
    assert pcpu.run_command(_RuleEngine(), ["-p", seq, "-q", stp] + base + ["-o", first, fa, st]) == 0
    assert pcpu.run_command(_RuleEngine(), ["-p", first + ".expected.seq.txt", "-q", first + ".expected.struct.txt"] + base + ["-o", second, fa, st]) == 0
    a, b, c = joint_outputs(two), joint_outputs(first), joint_outputs(second)
    assert a[0] == c[0] and a[2:] == c[2:] and a[3] != b[3]


def test_option_refusals_before_anything_is_read(tmp_path, capsys):
    fa, d, st, data, order = make_inputs(tmp_path)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    prefix = str(tmp_path / "out")
    for argv in (["-q", stp, "--joint", d], ["-q", str(tmp_path / "none.pfm"), "--joint", str(tmp_path / "nowhere")]):
        assert pcpu.run_command(None, ["-o", prefix] + argv) == 1                 # engine None: a device would be opened if the check came later
        err = capsys.readouterr().err
        assert "--joint" in err and "-p" in err and "sequences" in err
    assert not any(os.path.exists(prefix + s) for s in (".expected.struct.txt", ".expected.seq.txt", ".expected.joint.txt", ".summary.txt"))


def test_the_non_finite_checks_run_structure_sequence_table(tmp_path, capsys):
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    prefix = str(tmp_path / "out")
    argv = ["-p", seq, "-q", stp, "-u", "-C", "0.01", "--joint", "-o", prefix, fa, d]

    def spoil(where):
        def f(stream, got):
            for i, r in where:
                got[i].reshape(got[i].shape[0], -1)[r, 1] = np.nan                    # a cell every matrix keeps
        return f
    # the table alone: its record; the table earlier than a matrix: the matrix's record is the one named (structure, sequence, table)
    for where, named in ((((2, 3),), order[3]), (((2, 0), (1, 4)), order[4]), (((2, 0), (1, 4), (0, 5)), order[5])):     # records in the FASTA's order
        for engine, merge in ((_RuleEngine, "host"), (_MergedEngine, "device")):
            assert pcpu.run_command(engine(spoil(where)), argv + ["--merge", merge]) == 1
            err = capsys.readouterr().err
            assert "Motif" in err and "record %s" % named in err and ("infinite" in err or "not a number" in err), (where, merge, err)
    assert not any(os.path.exists(prefix + s) for s in (".expected.struct.txt", ".expected.seq.txt", ".expected.joint.txt", ".summary.txt"))


def test_both_merge_routes_write_equal_bytes(tmp_path):
    """the device route with the merge's rules (exact integers) in the device's place"""
    from test_expect_merge_cpu import routes
    other = "EHTBLRM"
    fa, d, st, data, order = make_inputs(tmp_path)
    _, mixed, _, _, _ = make_inputs(tmp_path, orders=[FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER], name="mixed")
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4), seed=2, ids=["A", "B"])
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=3, ids=["A", "B"])
    for opts in (["-p", seq, "-q", stp], ["-p", seq]):
        for extra, source, fasta in ((["--all-motifs"], d, fa), (["--iterations", "2", "--batch-records", "3"], st, fa),
                                     (["--all-motifs", "--batch-records", "2"], mixed, str(tmp_path / "mixed.fa"))):
            routes(pcpu.run_command, joint_outputs, (_MergedEngine, _RuleEngine), opts + ["-u", "-C", "0.01", "--joint"] + extra, tmp_path, [fasta, source])
    ints = mrules.merge_ints(np.full((2, 1, 4, 8), 0.5))
    assert ints.shape == (1, 32) and mrules.rounded(ints).tolist() == [[1.0] * 32]


def test_a_negative_cell_mi_is_nan_and_the_device_route_refuses(tmp_path, capsys):
    from rnascan_amd import expect_profile
    from test_expect_merge_cpu import write_profile
    fa, d, st, data, order = make_inputs(tmp_path)
    rows = data["r3"][1].copy()
    rows[:, 2] = -5.0
    write_profile(d, "r3", rows)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    base = ["-p", seq, "-u", "-C", "0.01", "--weight", "ratio", "--joint"]
    assert pcpu.run_command(_RuleEngine(), base + ["--merge", "host", "-o", str(tmp_path / "host"), fa, d]) == 0
    header, got = joint_rows(str(tmp_path / "host") + ".expected.joint.txt")
    negative = [any(float(x) < 0 for x in r[1:29]) for r in got]
    assert any(negative) and [r[29] == "nan" for r in got] == negative
    assert math.isnan(expect_profile.mutual_information([[1.0, -0.5] + [0.0] * 5] * 4)) and expect_profile.mutual_information([[0.0] * 7] * 4) == 0.0
    capsys.readouterr()
    assert pcpu.run_command(_MergedEngine(), base + ["--merge", "auto", "-o", str(tmp_path / "auto"), fa, d]) == 0
    err = capsys.readouterr().err
    assert joint_outputs(tmp_path / "auto") == joint_outputs(tmp_path / "host") and "record r3" in err and "on the host" in err
    assert pcpu.run_command(_MergedEngine(), base + ["--merge", "device", "-o", str(tmp_path / "dev"), fa, d]) == 1
    assert "negative" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "dev") + ".expected.joint.txt")


# ---- the recorded outputs (tests/golden/expect_profile_joint): what the command wrote on the GPU, by both merge routes ----------
GOLDEN = os.path.join(REPO, "tests", "golden", "expect_profile_joint")
SUFFIXES = (".expected.struct.txt", ".summary.txt", ".expected.seq.txt", ".expected.joint.txt")      # joint_outputs' order
LIB_LENGTHS = (40, 3, 75, 130, 12, 260, 700, 33)


def golden(name):
    return tuple(open(os.path.join(GOLDEN, name + s)).read() for s in SUFFIXES)


def hist_inputs(tmp_path):
    """the histone 3' end with its averaged-structure profile as a directory of one file, and the two SLBP PFMs"""
    from rnascan_amd import fasta
    d = tmp_path / "avg"
    d.mkdir()
    fa = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
    shutil.copy(os.path.join(DATA_DIR, "HIST2H3C_3p_end_structure.txt"), str(d / ("structure.%s.txt" % fasta.open_lazy(fa).ids[0])))
    return (fa, str(d), os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt"),
            os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt"))


def test_the_recorded_outputs_are_the_rules(tmp_path):
    """the fixtures of tests/test_gpu_expect_profile_joint_cli.py, byte for byte, with the rules in the device's place"""
    fa, d, seq, stp = hist_inputs(tmp_path)
    for name, opts in (("hist_joint", ["-p", seq, "-q", stp]), ("hist_seq", ["-p", seq])):
        assert pcpu.run_command(_RuleEngine(), opts + ["-u", "-C", "0", "--joint", "-o", str(tmp_path / name), fa, d]) == 0
        assert joint_outputs(tmp_path / name) == golden(name)
    (tmp_path / "lib").mkdir()
    fa, d, st, data, order = make_inputs(tmp_path / "lib", lengths=LIB_LENGTHS)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4, 6), seed=2, ids=["A", "B", "C"])
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4, 6), seed=3, ids=["A", "B", "C"])
    assert pcpu.run_command(_RuleEngine(), ["-p", seq, "-q", stp, "-u", "-C", "0.01", "--all-motifs", "--joint", "-o", str(tmp_path / "library"), fa, d]) == 0
    assert joint_outputs(tmp_path / "library") == golden("library")
    argv = ["-p", seq, "-q", stp, "-C", "0.02", "--all-motifs", "--joint", "--weight", "ratio", "--iterations", "2"]
    assert pcpu.run_command(_MergedEngine(), argv + ["--merge", "device", "-o", str(tmp_path / "two"), fa, st]) == 0
    assert joint_outputs(tmp_path / "two") == golden("two")
