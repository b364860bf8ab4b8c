"""Expected counts on averaged-structure profiles on a GPU-less host: the rules (tests/expect_profile_rules.py) against the
letter rules they must reduce to, what the GPU tests' inputs tell apart, the bindings, and the command's host logic with the
rules standing in for the device."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import expect_profile_rules as rules
import expect_rules as erules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import test_occupancy_profile_cpu as occ_cpu
from conftest import REPO
from test_occupancy_profile_cpu import FILE_ORDER, STRUCT, make_inputs, write_pfm

MODES = (rules.RATIO, rules.POSTERIOR)


# ---- the rules against the letter rules --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", MODES)
def test_one_hot_rows_give_the_expected_letter_counts(dtype, mode):
    """w * 1 is w and w * 0 is +0.0 for the finite, non-negative weights of a finite table: on rows with a single 1 the
    structure matrix, the occupancy and Windows are expect_rules.expected of the structure letters, bit for bit"""
    rng = np.random.default_rng(5)
    for m in (1, 4, 9):
        letters, off, lens = orules.stream(rng, [int(x) for x in rng.integers(1, 200, size=10)] + [m - 1, m, m + 31, 1100], 7, case=True)
        S = prules.struct_table(rng, m)
        S[0, 2] = 0.0
        R7 = np.full((m, 8), np.nan)
        R7[:, :7] = S
        got = rules.expected(prules.one_hot(letters, dtype), off, lens, S, mode=mode)
        want = erules.expected(letters, off, lens, R7, 7, mode)
        assert got[1] is None and rules.same_bits(got[0], want[0]) and rules.same_bits(got[2], want[1]) and np.array_equal(got[3], want[2])
        assert (got[0][:, :, :, 7] == 0).all() and (got[0][:, 0] > 0).any()


@pytest.mark.parametrize("mode", MODES)
def test_sequence_tables_alone_give_the_letters_expected_counts(mode):
    """seq_tables only: exp_seq, occ and Windows are expect_rules.expected of the codes; the profile only enters exp_struct"""
    rng = np.random.default_rng(6)
    m = 6
    codes, profile, off, lens = prules.stream(rng, [40, m - 1, m, 300, 77, 1030], np.float32, foreign=0.01)
    R = np.stack([orules.table(rng, m) for _ in range(2)])
    got = rules.expected(profile, off, lens, None, codes, R, mode)
    want = erules.expected(codes, off, lens, R, 4, mode)
    assert rules.same_bits(got[1], want[0]) and rules.same_bits(got[2], want[1]) and np.array_equal(got[3], want[2])
    assert np.isfinite(got[0]).all() and (got[0][[0, 3, 4, 5]] > 0).any(axis=(1, 2, 3)).all() and (got[0][1] == 0).all()


# ---- what the GPU tests' inputs tell apart -----------------------------------------------------------------------------
def _contracted(profile, off, length, S, codes, R, mode):
    """exp_struct of one record if s + w * r were contracted: the product exact, one rounding after the addition (an FMA).
    The first product of a block is rounded on its own, as a multiplication is; levels 1 and up have no products."""
    t, has = prules.terms(profile, off, length, S, codes, R)
    w = erules.weights(t, has, orules.tree(t), mode)
    x = np.asarray(profile[int(off):int(off) + int(length)]).astype(np.float64)
    m, n_win = S.shape[0], t.size
    E = np.zeros((m, 8))
    for k in range(m):
        for c in range(7):
            sums = []
            for b0 in range(0, n_win, 32):
                s = None
                for i in range(b0, min(b0 + 32, n_win)):
                    if s is None:
                        s = float(w[i] * x[i + k, c]) if has[i] else 0.0
                    elif has[i]:
                        s = float(Fraction(s) + Fraction(float(w[i])) * Fraction(float(x[i + k, c])))
                sums.append(s)
            E[k, c] = orules.tree(np.asarray(sums)) if len(sums) > 1 else sums[0]
    return E


def _division_per_window(t, has, occ, mode):
    with np.errstate(all="ignore"):
        return np.where(has, np.asarray(t, dtype=np.float64) / np.float64(occ), 0.0) if mode == rules.POSTERIOR and occ != 0 else erules.weights(t, has, occ, mode)


def _from_zero(X):
    """expect_rules.tree_rows with every block started from 0.0 + instead of copying its first value"""
    a = np.asarray(X, dtype=np.float64)
    while a.shape[1] > 1:
        pad = (-a.shape[1]) % 32
        a = np.concatenate([a, np.zeros((a.shape[0], pad))], axis=1).reshape(a.shape[0], -1, 32)
        s = 0.0 + a[:, :, 0]
        for i in range(1, 32):
            s = s + a[:, :, i]
        a = s
    return 0.0 + a[:, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("joint", [False, True])
def test_the_gpu_inputs_tell_the_mistakes_apart(joint, dtype):
    """the base case of tests/test_gpu_expect_profile.py gives OTHER bits under a contracted w * r, a reversed stored column
    order, a window shifted by one and a division per window; a -0.0 cell shows a block that starts from 0.0 +"""
    codes, profile, off, lens, st, sq = prules.base_case(dtype=dtype)
    c, q = (codes, sq) if joint else (None, None)
    long = [0, 3, 4]                                                    # records with more than one window
    for mode in MODES:
        right = rules.expected(profile, off, lens, st, c, q, mode)[0]
        assert np.isfinite(right).all() and (right[long][:, :, :, :7] > 0).all() and (right[1] == 0).all()
        wrong = {
            "reversed columns": rules.expected(profile[:, ::-1], off, lens, st[:, :, ::-1], c, q, mode)[0][:, :, :, [6, 5, 4, 3, 2, 1, 0, 7]],
            "shifted window": rules.expected(np.roll(profile, -1, axis=0), off, lens, st, c, q, mode)[0],
            "contracted": np.stack([np.stack([_contracted(profile, o, n, st[k], c, None if q is None else q[k], mode) for k in range(st.shape[0])])
                                    for o, n in zip(off[long], lens[long])]),
        }
        if mode == rules.POSTERIOR:
            wrong["division per window"] = rules.expected(profile, off, lens, st, c, q, mode, weights=_division_per_window)[0]
        for name, got in wrong.items():
            if name != "contracted":
                got = got[long]
            differs = got.view(np.uint64) != right[long].view(np.uint64)
            assert differs.any(axis=(1, 2, 3)).all(), name              # every long record has a cell with other bits
            assert np.allclose(got, right[long], rtol=1e-9) or name == "shifted window", name   # ... of the same quantity
    # a column of -0.0 under 32 windows and under a lone window: copied it stays -0.0, added to 0.0 it does not
    m = st.shape[1]
    rng = np.random.default_rng(8)
    _, p2, o2, l2 = prules.stream(rng, [m + 31, m], dtype)
    p2[:, 3] = -0.0
    good = rules.expected(p2, o2, l2, st[0], mode=rules.RATIO)[0]
    bad = rules.expected(p2, o2, l2, st[0], mode=rules.RATIO, tree_rows=_from_zero)[0]
    assert np.signbit(good[:, 0, :, 3]).all() and (good[:, 0, :, 3] == 0).all() and not np.signbit(bad[:, 0, :, 3]).any()
    assert rules.same_bits(np.delete(good, 3, axis=3), np.delete(bad, 3, axis=3))
    # ... and padded anywhere (33 windows) the rules' sum is +0.0
    _, p3, o3, l3 = prules.stream(rng, [m + 32, m + 63], dtype)
    p3[:, 3] = -0.0
    assert not np.signbit(rules.expected(p3, o3, l3, st[0], mode=rules.RATIO)[0][:, 0, :, 3]).any()


# ---- bindings ----------------------------------------------------------------------------------------------------------
def test_abi_24_exports_the_expect_profile_entry_points():
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    assert _lib.ABI_VERSION >= 24 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) >= 24
    for name in ("pfmscan_expect_profile_dev", "pfmscan_expect_profile_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
    assert "pfmscan_expect_profile.hip" in build.SOURCES
    assert callable(_lib.Context.expect_profile_dev) and callable(_lib.Context.expect_profile_staged)
    assert callable(scanner.HipEngine.expect_profile)
    with pytest.raises(ValueError):
        _lib.Context._expect_profile_tables(None, None)


# ---- the command with the rules in the device's place ------------------------------------------------------------------
class _RuleEngine(occ_cpu._RuleEngine):
    """HipEngine.expect_profile answered by the rules (profile_colsums: the occupancy tests' engine)"""

    def expect_profile(self, stream, struct_tables, seq_tables, mode):
        self.calls.append((len(stream.offsets), stream.profile.dtype))
        return rules.expected(stream.profile, stream.offsets, stream.lengths, struct_tables, stream.codes, seq_tables, mode)


def run_command(engine, argv):
    from rnascan_amd import expect_profile
    return expect_profile.main(argv, engine=engine)


def outputs(prefix, seq=True):
    names = [".expected.struct.txt", ".summary.txt"] + ([".expected.seq.txt"] if seq else [])
    out = []
    for n in names:
        with open(str(prefix) + n) as f:
            out.append(f.read())
    return tuple(out)


def rule_sums(data, ids, struct_odds, seq_odds, mode, orders=None):
    """the matrices of the records ``ids`` by the rules, each record in ITS stored column order, mapped to FILE_ORDER (the
    written order) and added exactly -> (E_struct [m][7] in FILE_ORDER, E_seq [m][4] | None, occupancies)"""
    per_s, per_q, occs = [], [], []
    for sid in ids:
        seq, rows = data[sid]
        cols = orders[int(sid[1:])] if orders else FILE_ORDER
        profile = np.ascontiguousarray(rows[:, [STRUCT.index(c) for c in cols]])
        S = None if struct_odds is None else np.stack([struct_odds[c] for c in cols], axis=1)
        codes = np.array(["ACGU".index(c) if c in "ACGU" else 7 for c in seq], dtype=np.uint8)
        R = None if seq_odds is None else seq_odds.ratio_table("ACGU")
        es, eq, occ, _ = rules.expected_record(profile, 0, len(seq), S, codes, R, mode)
        per_s.append(es[:, [cols.index(c) for c in FILE_ORDER]])
        per_q.append(eq)
        occs.append(occ)
    m = per_s[0].shape[0]
    Es = np.array([[math.fsum(e[k, c] for e in per_s) for c in range(7)] for k in range(m)])
    Eq = None if seq_odds is None else np.array([[math.fsum(e[k, c] for e in per_q) for c in range(4)] for k in range(m)])
    return Es, Eq, occs


def read_matrix(path, letters):
    from rnascan_amd import pssm
    got = pssm.read_pfm(path)
    assert list(got.keys()) == list(letters)
    return np.stack([got[l] for l in letters], axis=1)


@pytest.mark.parametrize("weight", ["posterior", "ratio"])
def test_command_three_forms_directory_store_batches_and_order(tmp_path, weight):
    from rnascan_amd import expect, pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.01, "GAUC", None).values()))
    mode = expect.MODES[weight]
    base = ["-u", "-C", "0.01", "--weight", weight]
    forms = {"struct": (["-q", stp], [d], s_odds, None), "joint": (["-p", seq, "-q", stp], [fa, d], s_odds, q_odds),
             "seq": (["-p", seq], [fa, d], None, q_odds)}
    for name, (opts, inputs, so, qo) in forms.items():
        prefix = str(tmp_path / name)
        assert run_command(_RuleEngine(), opts + base + ["-o", prefix] + inputs) == 0
        got = outputs(prefix, seq=qo is not None)
        assert os.path.exists(prefix + ".expected.seq.txt") == (qo is not None)
        Es, Eq, occs = rule_sums(data, sorted(data), so, qo, mode)
        assert read_matrix(prefix + ".expected.struct.txt", FILE_ORDER).tolist() == Es.tolist()
        if qo is not None:
            assert read_matrix(prefix + ".expected.seq.txt", "ACGU").tolist() == Eq.tolist()
        lines = got[1].splitlines()
        assert lines[0].split("\t") == expect.COLUMNS and len(lines) == 2
        row = lines[1].split("\t")
        counted = [o for o in occs if o > 0]
        assert row[1:4] == ["1", str(len(counted)), str(len(occs) - len(counted))] and len(counted) == 5      # r1 is 3 long
        assert row[5] == repr(round(math.fsum(math.log2(o) for o in counted), 3))
        windows = sum(max(len(data[s][0]) - 5, 0) for s in data) - (6 if qo is not None else 0)   # r2's windows over the N
        assert int(row[4]) == windows
        # the written files are PFMs that -q / -p read; batches, the store and (with a FASTA) the record order change no byte
        assert pssm.load_odds(prefix + ".expected.struct.txt", 0.01, "EHTBLRM", None)
        for extra, inp in ((["--batch-records", "1"], inputs), (["--batch-records", "4"], inputs), ([], inputs[:-1] + [st]),
                           (["--batch-records", "2"], inputs[:-1] + [st])):
            e = _RuleEngine()
            other = str(tmp_path / "other")
            assert run_command(e, opts + base + extra + ["-o", other] + inp) == 0
            assert outputs(other, seq=qo is not None) == got
            if extra == ["--batch-records", "1"]:
                assert len(e.calls) == 6
        if qo is not None:
            blocks = open(fa).read().strip().split("\n>")
            (tmp_path / "rev.fa").write_text(">" + "\n>".join(b.lstrip(">") for b in reversed(blocks)) + "\n")
            assert run_command(_RuleEngine(), opts + base + ["-o", str(tmp_path / "rev"), str(tmp_path / "rev.fa"), d]) == 0
            assert outputs(tmp_path / "rev") == got
    if weight == "posterior":                                         # one site per counted record: a row of the profile sums to ~1
        E = read_matrix(str(tmp_path / "struct") + ".expected.struct.txt", FILE_ORDER)
        assert np.allclose(E.sum(axis=1), 5, atol=1e-4)
        E = read_matrix(str(tmp_path / "seq") + ".expected.seq.txt", "ACGU")
        assert np.allclose(E.sum(axis=1), 5, atol=1e-9)


@pytest.mark.parametrize("form", ["struct", "joint", "seq"])
def test_windows_column_of_a_library_of_mixed_widths(tmp_path, form):
    """Windows is the number of windows with a term: it depends on the motif's width, and with -p on the codes (r2 holds
    one N).  Every motif of a mixed-width library gets ITS figure, whatever the order of the widths and the batch size"""
    from rnascan_amd import pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    widths, ids = (6, 4, 6, 3), ["A", "B", "C", "D"]
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", widths, seed=2, ids=ids)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, widths, seed=3, ids=ids)
    opts = (["-p", seq] if form != "struct" else []) + (["-q", stp] if form != "seq" else [])
    inputs = [st] if form == "struct" else [fa, st]
    s_odds, q_odds = pssm.load_odds(stp, 0.01, "EHTBLRM", None), pssm.load_odds(seq, 0.01, "GAUC", None)
    for extra in ([], ["--batch-records", "2"]):
        prefix = str(tmp_path / "out")
        assert run_command(_RuleEngine(), opts + ["-u", "-C", "0.01", "--all-motifs"] + extra + ["-o", prefix] + inputs) == 0
        rows = [ln.split("\t") for ln in outputs(prefix, seq=form != "struct")[1].splitlines()[1:]]
        assert [r[0] for r in rows] == ids
        for r, m in zip(rows, widths):
            n_win = sum(max(len(data[sid][0]) - m + 1, 0) for sid in data)
            assert int(r[4]) == n_win - (m if form != "struct" else 0)          # the m windows over r2's N have no term
            occs = rule_sums(data, sorted(data), s_odds[r[0]] if form != "seq" else None, q_odds[r[0]] if form != "struct" else None,
                             rules.POSTERIOR)[2]
            assert int(r[2]) == sum(o > 0 for o in occs) and int(r[3]) == sum(not o > 0 for o in occs)
        assert len(set(r[4] for r in rows)) == 3                              # 6, 4 and 3 wide: three figures


def test_command_two_column_orders_in_one_directory(tmp_path):
    """files of two stored column orders: every run's matrix is mapped to the profile's letters before the records are added"""
    from rnascan_amd import pssm
    other = "EHTBLRM"
    orders = [FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER]
    fa, mixed, _, data, order = make_inputs(tmp_path, orders=orders, name="mixed")
    (tmp_path / "one").mkdir()
    _, plain, _, _, _ = make_inputs(tmp_path / "one")
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.0, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.0, "GAUC", None).values()))
    for opts, inp, so, qo in ((["-q", stp], [], s_odds, None), (["-p", seq, "-q", stp], [fa], s_odds, q_odds), (["-p", seq], [fa], None, q_odds)):
        assert run_command(_RuleEngine(), opts + ["-u", "-o", str(tmp_path / "m")] + inp + [mixed]) == 0
        assert run_command(_RuleEngine(), opts + ["-u", "-o", str(tmp_path / "p")] + inp + [plain]) == 0
        got = read_matrix(str(tmp_path / "m") + ".expected.struct.txt", FILE_ORDER)
        want = read_matrix(str(tmp_path / "p") + ".expected.struct.txt", FILE_ORDER)
        assert got.tolist() == rule_sums(data, sorted(data), so, qo, rules.POSTERIOR, orders)[0].tolist()
        assert want.tolist() == rule_sums(data, sorted(data), so, qo, rules.POSTERIOR)[0].tolist()
        assert np.allclose(got, want, rtol=1e-12)
        if so is not None:
            assert got.tolist() != want.tolist()                      # the marginal adds in the stored column order
        else:
            assert got.tolist() == want.tolist()                      # sequence weights: no sum runs over the columns
        for n in ("1", "2"):
            assert run_command(_RuleEngine(), opts + ["-u", "--batch-records", n, "-o", str(tmp_path / "b")] + inp + [mixed]) == 0
            assert outputs(tmp_path / "b", seq=qo is not None) == outputs(tmp_path / "m", seq=qo is not None)


@pytest.mark.parametrize("form", ["struct", "joint", "seq"])
def test_two_iterations_are_two_chained_runs(tmp_path, form):
    fa, d, st, data, order = make_inputs(tmp_path)
    for extra, widths in ((["--all-motifs"], (6, 4)), ([], (6,))):
        seq = write_pfm(tmp_path / ("seq%d.pfm" % len(widths)), "ACGU", widths, seed=2, ids=["A", "B"])
        stp = write_pfm(tmp_path / ("st%d.pfm" % len(widths)), STRUCT, widths, seed=3, ids=["A", "B"])
        base = ["-C", "0.02"] + extra
        inp = [st] if form == "struct" else [fa, st]
        files = lambda s, q: (["-p", s] if form != "struct" else []) + (["-q", q] if form != "seq" else [])
        first, second, two = str(tmp_path / "first"), str(tmp_path / "second"), str(tmp_path / "two")
        assert run_command(_RuleEngine(), files(seq, stp) + base + ["--iterations", "2", "-o", two] + inp) == 0
        assert run_command(_RuleEngine(), files(seq, stp) + base + ["-o", first] + inp) == 0
        assert run_command(_RuleEngine(), files(first + ".expected.seq.txt", first + ".expected.struct.txt") + base + ["-o", second] + inp) == 0
        with_seq = form != "struct"
        a, b, c = outputs(two, with_seq), outputs(first, with_seq), outputs(second, with_seq)
        assert a[0] == c[0] and a[2:] == c[2:]
        assert (a[2] != b[2]) if with_seq else (a[0] != b[0])
        rows = [ln.split("\t") for ln in a[1].splitlines()[1:]]
        w = len(widths)
        assert [r[1] for r in rows] == ["1"] * w + ["2"] * w
        assert [r[2:] for r in rows[:w]] == [ln.split("\t")[2:] for ln in b[1].splitlines()[1:]]
        assert [r[2:] for r in rows[w:]] == [ln.split("\t")[2:] for ln in c[1].splitlines()[1:]]
        if extra:
            assert [r[0] for r in rows[:w]] == ["A", "B"] and a[0].startswith("#A\n#PO\t" + "\t".join(FILE_ORDER))


def test_errors_before_a_device_is_opened(tmp_path, capsys):
    """exit 1, a message that names the cause, nothing written; engine None: a device would be opened (and fail here) if the
    check came later"""
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    seq5 = write_pfm(tmp_path / "seq5.pfm", "ACGU", (5,))
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    wide = write_pfm(tmp_path / "wide.pfm", STRUCT, (65,))
    prefix = str(tmp_path / "out")
    for argv, needles in (([d], ("-p", "-q")),
                          (["-q", stp, fa], ("not an averaged-structure", "rnascan_amd.expect")),
                          (["-p", seq, "-q", stp, d, fa], ("not an averaged-structure",)),
                          (["-p", seq, fa], ("-p needs the sequence FASTA",)),
                          (["-p", seq, d, st], ("sequence FASTA first",)),
                          (["-q", stp, fa, d], ("-q alone takes one input",)),
                          (["-q", stp, "--iterations", "0", d], ("--iterations", "at least 1")),
                          (["-q", stp, "--iterations", "2", "--pairing", "positional", d], ("--iterations", "positional")),
                          (["-q", wide, "-u", d], ("-q", "PFMSCAN_MAX_M", "65")),
                          (["-p", seq5, "-q", stp, fa, d], ("share no window",)),
                          (["-q", str(tmp_path / "none.pfm"), d], ("none.pfm",))):
        rc = run_command(None, ["-o", prefix] + argv)
        err = capsys.readouterr().err
        assert rc == 1, argv
        for needle in needles:
            assert needle in err, (argv, err)
        assert not any(os.path.exists(prefix + s) for s in (".expected.struct.txt", ".expected.seq.txt", ".summary.txt"))


def test_errors_after_the_pass(tmp_path, capsys):
    fa, d, st, data, order = make_inputs(tmp_path)
    prefix = str(tmp_path / "out")
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    # a background of 0 for a letter the motif has: a ratio is +inf, and the first record's occupancy with it
    bg = tmp_path / "bg.txt"
    bg.write_text("{'A': 0.0, 'C': 0.3, 'G': 0.3, 'U': 0.4}")
    for opts in (["-p", seq], ["-p", seq, "-q", stp, "-B", str(tmp_path / "bgs.txt")]):
        (tmp_path / "bgs.txt").write_text(repr(dict(zip(STRUCT, (0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1)))))
        assert run_command(_RuleEngine(), opts + ["-C", "0.01", "-b", str(bg), "-o", prefix, fa, d]) == 1
        err = capsys.readouterr().err
        assert "Motif seq" in err and "record r" in err and ("infinite" in err or "not a number" in err)
    # a motif no record contributes to: every window of every record meets a zero
    with open(str(tmp_path / "zero.pfm"), "w") as f:
        f.write("PO\tA\tC\tG\tU\n0\t1\t1\t1\t1\n1\t0\t0\t0\t0\n")
    assert run_command(_RuleEngine(), ["-p", str(tmp_path / "zero.pfm"), "-u", "-o", prefix, fa, d]) == 1
    err = capsys.readouterr().err
    assert "Motif zero" in err and "no record contributes" in err
    # a record whose length is not its profile's
    lines = open(fa).read().splitlines()
    lines[1] = lines[1] + "A"
    (tmp_path / "long.fa").write_text("\n".join(lines) + "\n")
    assert run_command(_RuleEngine(), ["-p", seq, "-u", "-o", prefix, str(tmp_path / "long.fa"), d]) == 1
    assert "letters long but its averaged-structure profile has" in capsys.readouterr().err
    assert not any(os.path.exists(prefix + s) for s in (".expected.struct.txt", ".expected.seq.txt", ".summary.txt"))
