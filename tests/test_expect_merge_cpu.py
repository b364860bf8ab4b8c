"""The device-side merge of the expected counts on a GPU-less host: the rules (tests/expect_merge_rules.py) against
math.fsum, the bindings, and the three commands' ``--merge`` routes with rule engines whose ``*_merged`` methods are made of
the rules and the library's host helpers."""
import math
import os
import re

import numpy as np
import pytest

import expect_merge_rules as mrules
import sites_lib_rules as lrules
import test_expect_cpu as ecpu
import test_expect_profile_cpu as pcpu
import test_pair_cpu as qcpu
from conftest import REPO
from test_occupancy_profile_cpu import FILE_ORDER, STRUCT, make_inputs, write_profile

RNA = "ACGU"


def draw(rng, shape, lo=0, hi=2046):
    """finite doubles >= 0 by bit pattern, exponent field uniform in [lo, hi]; some fractions end in 32 ones"""
    E = rng.integers(lo, hi + 1, size=shape, dtype=np.uint64)
    f = rng.integers(0, 1 << 52, size=shape, dtype=np.uint64)
    f = np.where(rng.random(shape) < 0.25, f | np.uint64(0xffffffff), f)
    return ((E << np.uint64(52)) | f).view(np.float64)


# ---- the rules -------------------------------------------------------------------------------------------------------
def test_rounding_is_fsum_below_overflow():
    rng = np.random.default_rng(1)
    for n_rec, hi in ((1, 2046), (7, 2040), (300, 2030), (300, 60)):
        exp = draw(rng, (n_rec, 2, 3, 8), 0, hi)
        exp[rng.random(exp.shape) < 0.2] = 0.0
        exp[0, 0, 0, 0], exp[0, 0, 0, 1] = 5e-324, -0.0
        A = mrules.merge_ints(exp)
        got, want = mrules.rounded(A), mrules.fsum_cells(exp)
        assert got.tobytes() == want.tobytes()
        limbs = mrules.limbs_of(A)
        assert lrules.normalised(limbs) and (lrules.acc_int(limbs) == A).all()


def test_special_values_of_the_rules():
    dbl_max = np.finfo(np.float64).max
    exp = np.zeros((3, 1, 1, 8))
    exp[:, 0, 0, 0] = dbl_max                                            # beyond DBL_MAX: +inf
    exp[:, 0, 0, 1] = [2.0 ** -1074, 2.0 ** -1074, 0.0]
    exp[:, 0, 0, 2] = [-0.0, 0.0, -0.0]
    exp[:, 0, 0, 3] = [1.0, 2.0 ** -53, 2.0 ** -53]                       # a tie broken by the third value
    exp[:, 0, 0, 4] = [1.0, 2.0 ** -53, 0.0]                              # a tie: to even
    got = mrules.rounded(mrules.merge_ints(exp))[0]
    assert np.isposinf(got[0]) and got[1] == 1e-323 and got[2] == 0 and not np.signbit(got[2])
    assert got[3] == 1.0 + 2.0 ** -52 and got[4] == 1.0
    # rejected cells add nothing and name the smallest record; -0.0 is not negative
    exp = np.ones((5, 3, 2, 8))
    exp[3, 0, 1, 2], exp[1, 0, 0, 0], exp[2, 1, 0, 5], exp[4, 1, 1, 1], exp[0, 2, 0, 0], exp[2, 2, 0, 0] = np.nan, np.inf, -1.0, -3.5, -0.0, -np.inf
    assert mrules.bad(exp).tolist() == [[1, -1], [-1, 2], [2, 2]]
    A = mrules.merge_ints(exp)
    one = lrules.as_int(1.0)
    assert A[0, 0] == 4 * one and A[0, 10] == 4 * one and A[1, 5] == 4 * one and A[2, 0] == 3 * one and A[0, 1] == 5 * one
    assert mrules.bad(exp, before=[[0, 7], [-1, 3], [5, 1]]).tolist() == [[0, 7], [-1, 2], [2, 1]]


# ---- bindings --------------------------------------------------------------------------------------------------------
def test_abi_26_exports_the_merge_entry_points():
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    assert _lib.ABI_VERSION >= 26 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) >= 26
    assert int(re.search(r"#define\s+PFMSCAN_SITE_LIMBS\s+(\d+)", text).group(1)) == _lib.SITE_LIMBS == mrules.LIMBS
    for name in ("pfmscan_expect_merge_dev", "pfmscan_expect_merged_staged", "pfmscan_expect_profile_merged_staged", "pfmscan_expect_pair_merged_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
    assert "expected counts: the records added up on the device" in text and "zero_first" in text
    assert "pfmscan_expect_merge.hip" in build.SOURCES
    for name in ("expect_merge_dev", "expect_merged_staged", "expect_profile_merged_staged", "expect_pair_merged_staged"):
        assert callable(getattr(_lib.Context, name))
    for name in ("expect_merged", "expect_profile_merged", "expect_pair_merged"):
        assert callable(getattr(scanner.HipEngine, name))
    with pytest.raises(ValueError):
        _lib.Context._merge_acc(np.zeros((2, _lib.SITE_LIMBS, 8 * 5), dtype=np.uint64), 2, 6, "acc")
    with pytest.raises(ValueError):
        _lib.Context._merge_acc(np.zeros((2, _lib.SITE_LIMBS, 8 * 6), dtype=np.int64), 2, 6, "acc")


def test_host_helpers_round_and_add_as_the_rules_do():
    from rnascan_amd import _lib
    rng = np.random.default_rng(2)
    exp = draw(rng, (40, 2, 2, 8))
    exp[:, 0, 0, 0] = np.finfo(np.float64).max
    A = mrules.merge_ints(exp)
    acc = np.zeros((2, mrules.LIMBS, 16), dtype=np.uint64)
    for a, b in ((0, 11), (11, 12), (12, 40)):
        _lib.site_acc_add(acc, mrules.limbs_of(mrules.merge_ints(exp[a:b])))
    assert (acc == mrules.limbs_of(A)).all()
    got = _lib.site_acc_round(acc)
    assert got.tobytes() == mrules.rounded(A).tobytes() and np.isposinf(got[0, 0])


# ---- the commands with the rules in the device's place ------------------------------------------------------------------
def merge_into(acc, exp):
    """what a *_merged_staged call does with the matrices exp of its records: acc += their exact sum; -> bad"""
    from rnascan_amd import _lib
    _lib.site_acc_add(acc, mrules.limbs_of(mrules.merge_ints(exp)))
    return mrules.bad(exp)


class MergedEngine(ecpu._RuleEngine):
    def expect_merged(self, stream, ratio_tables, n_letters, mode, acc, which=0):
        e, o, w = self.expect(stream, ratio_tables, n_letters, mode, which)
        return merge_into(acc, e), o, w


class MergedProfileEngine(pcpu._RuleEngine):
    def expect_profile_merged(self, stream, struct_tables, seq_tables, mode, acc_struct, acc_seq=None):
        es, eq, o, w = self.expect_profile(stream, struct_tables, seq_tables, mode)
        return merge_into(acc_struct, es), (None if acc_seq is None else merge_into(acc_seq, eq)), o, w


class MergedPairEngine(qcpu._RuleEngine):
    def expect_pair_merged(self, stream, seq_tables, struct_tables, mode, acc_seq, acc_struct):
        eq, es, o, w = self.expect_pair(stream, seq_tables, struct_tables, mode)
        return merge_into(acc_seq, eq), merge_into(acc_struct, es), o, w


def routes(run, outputs, engines, argv, tmp_path, inputs):
    """the three settings on an engine with and one without the merged method: equal bytes"""
    merged, plain = engines
    assert run(plain(), argv + ["--merge", "host", "-o", str(tmp_path / "host")] + inputs) == 0
    want = outputs(tmp_path / "host")
    for engine, merge in ((merged(), "device"), (merged(), "auto"), (merged(), "host"), (plain(), "auto")):
        assert run(engine, argv + ["--merge", merge, "-o", str(tmp_path / "got")] + inputs) == 0
        assert outputs(tmp_path / "got") == want, merge
    return want


def test_expect_routes_write_equal_bytes(tmp_path, capsys):
    fa = tmp_path / "s.fa"
    fa.write_text(ecpu.FASTA)
    pfm = ecpu.write_pfm(tmp_path / "lib.pfm", RNA, (6, 4, 6), seed=5)
    for extra in (["--all-motifs"], ["--all-motifs", "--iterations", "2", "--weight", "ratio"], ["--batch-records", "1"], ["--batch-records", "3", "-u"]):
        routes(ecpu.run_command, ecpu.outputs, (MergedEngine, ecpu._RuleEngine), ["-p", pfm, "-C", "0.1"] + extra, tmp_path, [str(fa)])
    # an engine without the method cannot take --merge device
    assert ecpu.run_command(ecpu._RuleEngine(), ["-p", pfm, "--merge", "device", "-o", str(tmp_path / "x"), str(fa)]) == 1
    assert "--merge device" in capsys.readouterr().err


def test_expect_pair_routes_write_equal_bytes(tmp_path):
    fa, sfa = qcpu.write_inputs(tmp_path)
    seq = ecpu.write_pfm(tmp_path / "seq.pfm", RNA, (6, 4), seed=3)
    st = ecpu.write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=4)
    for extra in (["--all-motifs"], ["--all-motifs", "--iterations", "2"], ["--batch-records", "2", "--weight", "ratio"]):
        routes(qcpu.run_expect, qcpu.outputs, (MergedPairEngine, qcpu._RuleEngine),
               ["-p", seq, "-q", st, "-u", "-C", "0.02", "--struct-format", "letters"] + extra, tmp_path, [fa, sfa])


@pytest.mark.parametrize("form", ["struct", "joint", "seq"])
def test_expect_profile_routes_write_equal_bytes(tmp_path, form):
    other = "EHTBLRM"
    fa, d, st, data, order = make_inputs(tmp_path)
    _, mixed, _, _, _ = make_inputs(tmp_path, orders=[FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER], name="mixed")
    seq = pcpu.write_pfm(tmp_path / "seq.pfm", RNA, (6, 4), seed=2, ids=["A", "B"])
    stp = pcpu.write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=3, ids=["A", "B"])
    opts = (["-p", seq] if form != "struct" else []) + (["-q", stp] if form != "seq" else [])
    outputs = lambda prefix: pcpu.outputs(prefix, form != "struct")
    for extra, source, fasta in ((["--all-motifs"], d, fa), (["--iterations", "2", "--batch-records", "3"], st, fa),
                                 (["--all-motifs", "--batch-records", "2"], mixed, str(tmp_path / "mixed.fa")), (["--batch-records", "1"], mixed, str(tmp_path / "mixed.fa"))):
        routes(pcpu.run_command, outputs, (MergedProfileEngine, pcpu._RuleEngine), opts + ["-u", "-C", "0.01"] + extra, tmp_path,
               [source] if form == "struct" else [fasta, source])


def test_error_messages_name_the_same_record(tmp_path, capsys):
    fa = tmp_path / "s.fa"
    fa.write_text(ecpu.FASTA)
    prefix = str(tmp_path / "out")
    seq = ecpu.write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    bg = tmp_path / "bg.txt"
    bg.write_text("{'A': 0.0, 'C': 0.3, 'G': 0.3, 'U': 0.4}")
    said = []
    for engine, merge in ((ecpu._RuleEngine(), "host"), (MergedEngine(), "device"), (MergedEngine(), "auto")):
        for weight in ("posterior", "ratio"):                             # posterior: the occupancy is +inf; ratio: so are cells
            assert ecpu.run_command(engine, ["-p", seq, "-C", "0.01", "-b", str(bg), "--weight", weight, "--merge", merge, "-o", prefix, str(fa)]) == 1
            said.append(capsys.readouterr().err)
    assert len(set(said)) == 1 and "Motif seq" in said[0] and "record r1" in said[0]
    with open(str(tmp_path / "zero.pfm"), "w") as f:
        f.write("PO\tA\tC\tG\tU\n0\t1\t1\t1\t1\n1\t0\t0\t0\t0\n")
    said = []
    for engine, merge in ((ecpu._RuleEngine(), "host"), (MergedEngine(), "device")):
        assert ecpu.run_command(engine, ["-p", str(tmp_path / "zero.pfm"), "-u", "--merge", merge, "-o", prefix, str(fa)]) == 1
        said.append(capsys.readouterr().err)
    assert said[0] == said[1] and "no record contributes" in said[0]
    assert not os.path.exists(prefix + ".expected.txt") and not os.path.exists(prefix + ".summary.txt")


def test_a_cell_only_nonfinite_in_a_matrix_names_its_record(tmp_path, capsys):
    """ratio weights with an infinite ratio under a letter only r4 holds in that column: the occupancy check finds it first on
    both routes; with the occupancy hidden (an engine that reports finite occupancies) the matrices' verdict names the record"""
    class Hidden(MergedEngine):
        def expect(self, stream, ratio_tables, n_letters, mode, which=0):
            e, o, w = MergedEngine.expect(self, stream, ratio_tables, n_letters, mode, which)
            return e, np.where(np.isfinite(o), o, 1.0), w

    fa = tmp_path / "s.fa"
    fa.write_text(ecpu.FASTA)
    seq = ecpu.write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    bg = tmp_path / "bg.txt"
    bg.write_text("{'A': 0.0, 'C': 0.3, 'G': 0.3, 'U': 0.4}")
    said = []
    for merge in ("host", "device"):
        assert ecpu.run_command(Hidden(), ["-p", seq, "-C", "0.01", "-b", str(bg), "--weight", "ratio", "--merge", merge, "--batch-records", "2",
                                           "-o", str(tmp_path / "o"), str(fa)]) == 1
        said.append(capsys.readouterr().err)
    assert said[0] == said[1] and "record r1" in said[0]


def test_a_negative_profile_cell(tmp_path, capsys):
    """-u accepts negative profile cells: a record whose column is negative throughout has a negative expected count, which the
    host route sums and the device's accumulators cannot hold"""
    fa, d, st, data, order = make_inputs(tmp_path)
    rows = data["r3"][1].copy()
    rows[:, 2] = -0.05
    write_profile(d, "r3", rows)
    stp = pcpu.write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    base = ["-q", stp, "-u", "-C", "0.01"]
    assert pcpu.run_command(pcpu._RuleEngine(), base + ["--merge", "host", "-o", str(tmp_path / "host"), d]) == 0
    capsys.readouterr()
    assert pcpu.run_command(MergedProfileEngine(), base + ["--merge", "auto", "-o", str(tmp_path / "auto"), d]) == 0
    err = capsys.readouterr().err
    assert pcpu.outputs(tmp_path / "auto", False) == pcpu.outputs(tmp_path / "host", False)
    assert "record r3" in err and "negative" in err and "on the host" in err
    assert pcpu.run_command(MergedProfileEngine(), base + ["--merge", "device", "-o", str(tmp_path / "dev"), d]) == 1
    err = capsys.readouterr().err
    assert "Motif st" in err and "record r3" in err and "negative" in err and not os.path.exists(str(tmp_path / "dev") + ".summary.txt")


def test_a_sum_beyond_the_largest_double(tmp_path, capsys):
    """the device route rounds to +inf and says which motif; nothing is written"""
    class Huge(MergedEngine):
        def expect(self, stream, ratio_tables, n_letters, mode, which=0):
            e, o, w = MergedEngine.expect(self, stream, ratio_tables, n_letters, mode, which)
            return np.where(e > 0, np.finfo(np.float64).max, e), o, w

    fa = tmp_path / "s.fa"
    fa.write_text(ecpu.FASTA)
    seq = ecpu.write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    assert ecpu.run_command(Huge(), ["-p", seq, "-u", "-C", "0.01", "--merge", "device", "-o", str(tmp_path / "o"), str(fa)]) == 1
    err = capsys.readouterr().err
    assert "Motif seq" in err and "largest double" in err and not os.path.exists(str(tmp_path / "o") + ".expected.txt")


def write_zero_row_library(path, letters):
    """M0 (width 3, fine), M1 (width 2) and M2 (width 3), the second row of M1 and of M2 all zeros: under -u every ratio of
    that row is 0, so is every occupancy, and no record contributes to M1 or to M2"""
    with open(str(path), "w") as f:
        for k, m in enumerate((3, 2, 3)):
            f.write("#M%d\n#PO\t%s\n" % (k, "\t".join(letters)))
            for j in range(m):
                f.write("%d\t%s\n" % (j, "\t".join("0" if k and j == 1 else "1" for _ in letters)))
            f.write("\n")
    return str(path)


@pytest.mark.parametrize("route", ["host", "device"])
def test_which_motif_a_pass_without_a_contribution_names(tmp_path, capsys, route):
    """the order in which a pass finalises its motifs: ``expect`` by width group (groups by first appearance, so M0, M2, M1),
    ``expect_pair`` and ``expect_profile`` in file order (M0, M1, M2)"""
    seq = write_zero_row_library(tmp_path / "seq.pfm", RNA)
    st = write_zero_row_library(tmp_path / "st.pfm", STRUCT)
    engines = (ecpu._RuleEngine, qcpu._RuleEngine, pcpu._RuleEngine) if route == "host" else (MergedEngine, MergedPairEngine, MergedProfileEngine)
    opts = ["-u", "--all-motifs", "--merge", route, "-o", str(tmp_path / "out")]
    fa = tmp_path / "s.fa"
    fa.write_text(ecpu.FASTA)
    assert ecpu.run_command(engines[0](), ["-p", seq] + opts + [str(fa)]) == 1
    assert capsys.readouterr().err == "Motif M2: no record contributes (every occupancy is 0)\n"
    pfa, psfa = qcpu.write_inputs(tmp_path)
    assert qcpu.run_expect(engines[1](), ["-p", seq, "-q", st, "--struct-format", "letters"] + opts + [pfa, psfa]) == 1
    assert capsys.readouterr().err == "Motif M1: no record contributes (every occupancy is 0)\n"
    _, d, _, _, _ = make_inputs(tmp_path)
    assert pcpu.run_command(engines[2](), ["-q", st] + opts + [d]) == 1
    assert capsys.readouterr().err == "Motif M1: no record contributes (every occupancy is 0)\n"
