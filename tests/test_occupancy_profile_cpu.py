"""Occupancy on averaged-structure profiles on a GPU-less host: the rules (tests/occupancy_profile_rules.py) against the
letter-string rules and against exact rational arithmetic, what the GPU tests' inputs can tell apart, the bindings, and the
command's host logic with the rules standing in for the device."""
import io
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

import background_rules as brules
import occupancy_profile_rules as rules
import occupancy_rules as orules
from conftest import DATA_DIR, REPO

STRUCT = "EHTBLRM"                          # code order of structure letters (pack.STRUCT_LETTERS)
FILE_ORDER = "BEHLMRT"                      # column order of the averaged-structure files pfmutil writes


# ---- the rules against the letter-string rules -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_hot_rows_give_the_letter_occupancy(dtype):
    """1 * S + 0 * S ... = S exactly: structure only equals occupancy_rules.occupancy of the letter codes bit for bit
    (all-finite tables, a +0.0 cell among them); joint equals the product chain of both letter tables"""
    rng = np.random.default_rng(3)
    for m in (1, 4, 9):
        letters, off, lens = orules.stream(rng, [int(x) for x in rng.integers(1, 200, size=12)] + [m - 1, m, 700], 7)
        codes = rng.integers(0, 4, size=letters.size).astype(np.uint8)
        codes[rng.random(codes.size) < 0.02] = 5
        S = rules.struct_table(rng, m)
        S[0, 2] = 0.0
        R7 = np.full((m, 8), np.nan)
        R7[:, :7] = S
        P = rules.one_hot(letters, dtype)
        got = rules.occupancy(P, off, lens, S)
        want = orules.occupancy(letters, off, lens, R7, 7)
        assert rules.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
        R4 = orules.table(rng, m)
        got = rules.occupancy(P, off, lens, S, codes, R4)
        for r, (o, n) in enumerate(zip(off, lens)):
            n_win = max(int(n) - m + 1, 0)
            t = np.zeros(n_win)
            for s in range(n_win):
                c, l = codes[o + s:o + s + m] & 7, letters[o + s:o + s + m] & 7
                if (c >= 4).any():
                    continue
                x = R4[0, c[0]]
                for k in range(1, m):
                    x = x * R4[k, c[k]]
                for k in range(m):
                    x = x * S[k, l[k]]
                t[s] = x
            assert rules.same_bits(got[0][r, 0], orules.tree(t))


# ---- the rules against exact arithmetic --------------------------------------------------------------------------------
def exact_terms(profile, off, length, S, codes=None, R=None):
    m = S.shape[0]
    out = []
    for s in range(max(int(length) - m + 1, 0)):
        x = Fraction(1)
        for k in range(m):
            if R is not None:
                x *= Fraction(float(R[k, codes[off + s + k] & 7]))
            x *= sum(Fraction(float(profile[off + s + k, c])) * Fraction(float(S[k, c])) for c in range(7))
        out.append(x)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [1, 5, 12])
def test_terms_against_exact_rational_arithmetic(m, dtype):
    """a few hundred windows of non-negative rows: within gamma(8 m - 1) relative (structure only) and gamma(9 m - 1)
    (joint) of the exact value, the bounds derived in the rules"""
    rng = np.random.default_rng(50 + m)
    codes, profile, off, lens = rules.stream(rng, [150 + m, 100 + m], dtype)
    S, R = rules.struct_table(rng, m), orules.table(rng, m)
    seen = 0
    for joint in (False, True):
        bound = Fraction(rules.term_bound(m, joint))
        assert rules.term_bound(m, joint) == rules.gamma((9 if joint else 8) * m - 1)
        for o, n in zip(off, lens):
            t, has = rules.terms(profile, o, n, S, codes if joint else None, R if joint else None)
            assert has.all()
            for got, want in zip(t, exact_terms(profile, int(o), int(n), S, codes if joint else None, R if joint else None)):
                assert abs(Fraction(float(got)) - want) <= bound * want
                seen += 1
    assert seen == 2 * (151 + 101)


# ---- what the GPU tests' inputs tell apart -----------------------------------------------------------------------------
def _fma_marginal(rows, s):
    """the contracted form: each product exact and added before the one rounding (what an FMA would compute)"""
    x = np.asarray(rows).astype(np.float64)
    out = np.zeros(x.shape[0])
    for i in range(x.shape[0]):
        d = float(Fraction(float(x[i, 0])) * Fraction(float(s[0])))
        for c in range(1, 7):
            d = float(Fraction(d) + Fraction(float(x[i, c])) * Fraction(float(s[c])))
        out[i] = d
    return out


def _f32_marginal(rows, s):
    x, s = np.asarray(rows).astype(np.float32), np.asarray(s).astype(np.float32)
    d = x[:, 0] * s[0]
    for c in range(1, 7):
        d = d + x[:, c] * s[c]
    return d.astype(np.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("joint", [False, True])
def test_the_gpu_inputs_tell_the_mistakes_apart(joint, dtype):
    """the basic case of tests/test_gpu_occupancy_profile.py gives OTHER bits under a contracted marginal, float32
    accumulation, the reversed column order and a window shifted by one: any of these in the kernel fails the GPU test"""
    codes, profile, off, lens, st, sq = rules.base_case(dtype=dtype)
    c, q = (codes, sq) if joint else (None, None)
    right = rules.occupancy(profile, off, lens, st, c, q)[0]
    assert np.isfinite(right).all() and (right[[0, 2, 3, 4]] > 0).all() and (right[1] == 0).all()
    long = [0, 3, 4]                                                    # records with more than one window
    wrong = {
        "contracted": rules.occupancy(profile, off, lens, st, c, q, marg=_fma_marginal)[0],
        "float32": rules.occupancy(profile, off, lens, st, c, q, marg=_f32_marginal)[0],
        "reversed columns": rules.occupancy(profile, off, lens, st[:, :, ::-1], c, q)[0],
        "shifted window": rules.occupancy(np.roll(profile, -1, axis=0), off, lens, st, c, q)[0],
    }
    for name, got in wrong.items():
        differs = got[long].view(np.uint64) != right[long].view(np.uint64)
        assert differs.any(), name                                      # one cell with other bits fails test_base_case
        assert differs.all() or name == "contracted", name              # (a contracted sum often rounds to the same double)
    assert np.allclose(wrong["contracted"][long], right[long], rtol=1e-13)   # ... although it is the same quantity


# ---- bindings ----------------------------------------------------------------------------------------------------------
def test_abi_22_exports_the_profile_entry_points():
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    assert _lib.ABI_VERSION >= 22 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) >= 22
    for name in ("pfmscan_occupancy_profile_dev", "pfmscan_occupancy_profile_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
    assert hasattr(_lib.Context, "occupancy_profile_staged") and hasattr(_lib.Context, "occupancy_profile_dev")
    assert hasattr(scanner.HipEngine, "occupancy_profile")


# ---- the command with the rules in the device's place ------------------------------------------------------------------
class _RuleEngine(object):
    """HipEngine.occupancy and HipEngine.occupancy_profile answered by the rules"""

    def __init__(self):
        self.calls = []

    def occupancy(self, stream, ratio_tables, n_letters, which=0):
        return orules.occupancy(stream.codes2 if which else stream.codes, stream.offsets, stream.lengths, ratio_tables, n_letters)

    def occupancy_profile(self, stream, struct_tables, seq_tables=None):
        self.calls.append((len(stream.offsets), stream.profile.dtype))
        return rules.occupancy(stream.profile, stream.offsets, stream.lengths, struct_tables, stream.codes, seq_tables)

    def profile_colsums(self, stream):
        """HipEngine.profile_colsums by its rules (tests/background_rules.py): the default structure background"""
        bad = brules.first_bad(stream.profile, stream.offsets, stream.lengths)
        if bad >= 0:
            err = ValueError("bad cell")
            err.element = bad
            raise err
        return brules.colsums(stream.profile, stream.offsets, stream.lengths)

    def close(self):
        pass


def run_command(engine, argv):
    from rnascan_amd import occupancy
    out = io.StringIO()
    rc = occupancy.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def write_pfm(path, letters, widths, seed=0, ids=None):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for k, m in enumerate(widths):
            if len(widths) > 1:
                f.write("#%s\n#" % (ids[k] if ids else "M%d" % k))
            f.write("PO\t" + "\t".join(letters) + "\n")
            for j in range(m):
                f.write("%d\t%s\n" % (j, "\t".join("%.4f" % x for x in rng.dirichlet(np.full(len(letters), 0.6)))))
            f.write("\n")
    return str(path)


def write_profile(directory, sid, rows, order=FILE_ORDER):
    """rows [L][7] in EHTBLRM order -> structure.<sid>.txt with its columns in ``order``"""
    with open(os.path.join(str(directory), "structure.%s.txt" % sid), "w") as f:
        f.write("PO\t" + "\t".join(order) + "\n")
        for i, row in enumerate(rows):
            f.write("%d\t%s\n" % (i, "\t".join(repr(float(row[STRUCT.index(c)])) for c in order)))


def make_inputs(tmp_path, lengths=(40, 3, 75, 130, 12, 260), seed=1, orders=None, name="avg"):
    """a FASTA (ids r0 .. in an order that is NOT the sorted one), a profile directory, a store of it; -> paths + the data"""
    from rnascan_amd import store
    rng = np.random.default_rng(seed)
    d = tmp_path / name
    d.mkdir()
    data = {}
    ids = ["r%d" % i for i in range(len(lengths))]
    for i, (sid, n) in enumerate(zip(ids, lengths)):
        seq = "".join(rng.choice(list("ACGU"), size=n))
        if i == 2:
            seq = seq[:20] + "N" + seq[21:]
        data[sid] = (seq, np.round(rules.rows(rng, n), 6))
        write_profile(d, sid, data[sid][1], orders[i] if orders else FILE_ORDER)
    fa = tmp_path / (name + ".fa")
    order = ids[1::2] + ids[0::2]
    fa.write_text("".join(">%s some text\n%s\n" % (sid, data[sid][0]) for sid in order))
    st = None
    if not orders:
        st = str(tmp_path / (name + ".store"))
        store.build_store(str(d), st)
    return str(fa), str(d), st, data, order


def rule_cell(data, sid, struct_odds, seq_odds=None, cols=FILE_ORDER, dtype=np.float64):
    """the occupancy and Windows of one record as the rules give them for rows stored in column order ``cols``"""
    seq, rows = data[sid]
    profile = np.ascontiguousarray(rows[:, [STRUCT.index(c) for c in cols]]).astype(dtype)
    S = np.stack([struct_odds[c] for c in cols], axis=1)
    codes = np.array(["ACGU".index(c) if c in "ACGU" else 7 for c in seq], dtype=np.uint8)
    R = None if seq_odds is None else seq_odds.ratio_table("ACGU")
    occ, win = rules.occupancy(profile, [0], [len(seq)], S, codes, R)
    return occ[0, 0], int(win[0])


def rows_of(text):
    return [ln.split("\t") for ln in text.splitlines()[1:]]


def test_command_both_modes_directory_store_and_batches(tmp_path):
    from rnascan_amd import occupancy, pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.0, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.0, "GAUC", None).values()))
    # joint: the FASTA's order, which is not the profiles'
    e = _RuleEngine()
    rc, text = run_command(e, ["-p", seq, "-q", stp, "-u", fa, d])
    assert rc == 0 and text.splitlines()[0].split("\t") == occupancy.COLUMNS
    rows = rows_of(text)
    assert [r[1] for r in rows] == order and sorted(order) != order
    for r in rows:
        occ, win = rule_cell(data, r[1], s_odds, q_odds)
        assert r[3] == repr(float(occ)) and int(r[2]) == win and r[4] == occupancy.log2_text(occ)
    assert rows[order.index("r1")][2:] == ["0", "0.0", "-inf"]                       # 3 letters: shorter than the motif
    assert int(rows[order.index("r2")][2]) == 75 - 5 - 6                              # the windows over the N have no term
    assert all(dt == np.float64 for _, dt in e.calls)
    for n in ("1", "3"):
        assert run_command(_RuleEngine(), ["-p", seq, "-q", stp, "-u", "--batch-records", n, fa, d])[1] == text
    e = _RuleEngine()
    assert run_command(e, ["-p", seq, "-q", stp, "-u", "--batch-records", "1", fa, d])[1] == text and len(e.calls) == 6
    assert run_command(_RuleEngine(), ["-p", seq, "-q", stp, "-u", fa, st])[1] == text
    assert run_command(_RuleEngine(), ["-p", seq, "-q", stp, "-u", "--batch-records", "3", fa, st])[1] == text
    # structure only: every window inside a record has a term; the directory's order is the file system's, the store's is sorted
    rc, only = run_command(_RuleEngine(), ["-q", stp, "-u", d])
    assert rc == 0
    rows = rows_of(only)
    assert sorted(r[1] for r in rows) == sorted(order)
    for r in rows:
        occ, win = rule_cell(data, r[1], s_odds)
        assert r[3] == repr(float(occ)) and int(r[2]) == win == max(len(data[r[1]][0]) - 5, 0)
    for n in ("1", "3"):
        assert run_command(_RuleEngine(), ["-q", stp, "-u", "--batch-records", n, d])[1] == only
    rc, stored = run_command(_RuleEngine(), ["-q", stp, "-u", st])
    assert rc == 0 and [r[1] for r in rows_of(stored)] == sorted(order) and sorted(stored.splitlines()) == sorted(only.splitlines())
    assert run_command(_RuleEngine(), ["-q", stp, "-u", "--batch-records", "2", st])[1] == stored
    # -B: the structure background from a file; --profile-dtype: float32 rows give the float32 rule's values
    bg = tmp_path / "bg.txt"
    bg.write_text(repr(dict(zip(STRUCT, (0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1)))))
    b_odds = next(iter(pssm.load_odds(stp, 0.0, "EHTBLRM", dict(zip(STRUCT, (0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1)))).values()))
    e = _RuleEngine()
    rc, text = run_command(e, ["-q", stp, "-B", str(bg), "--profile-dtype", "float32", st])
    assert rc == 0 and all(dt == np.float32 for _, dt in e.calls)
    for r in rows_of(text):
        assert r[3] == repr(float(rule_cell(data, r[1], b_odds, dtype=np.float32)[0]))
    assert sorted(run_command(_RuleEngine(), ["-q", stp, "-B", str(bg), "--profile-dtype", "float32", d])[1].splitlines()) == sorted(text.splitlines())


def test_command_two_column_orders_in_one_directory(tmp_path):
    """files of two column orders: each record's value is the rule's for ITS stored order (the test computes both), against
    the same data written in one order"""
    from rnascan_amd import pssm
    other = "EHTBLRM"
    orders = [FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER]
    fa, mixed, _, data, order = make_inputs(tmp_path, orders=orders, name="mixed")
    (tmp_path / "one").mkdir()
    _, plain, _, data1, _ = make_inputs(tmp_path / "one")
    assert all(np.array_equal(data[k][1], data1[k][1]) and data[k][0] == data1[k][0] for k in data)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.0, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.0, "GAUC", None).values()))
    for argv, so in ((["-p", seq, "-q", stp, "-u", fa], q_odds), (["-q", stp, "-u"], None)):
        rc, got = run_command(_RuleEngine(), argv + [mixed])
        rc1, want = run_command(_RuleEngine(), argv + [plain])
        assert rc == 0 and rc1 == 0
        a, b = dict((r[1], r) for r in rows_of(got)), dict((r[1], r) for r in rows_of(want))
        assert sorted(a) == sorted(b) == sorted(order)
        other_bits = 0
        for sid, r in a.items():
            cols = orders[int(sid[1:])]
            occ, win = rule_cell(data, sid, s_odds, so, cols)
            assert r[3] == repr(float(occ)) and int(r[2]) == win == int(b[sid][2])
            assert b[sid][3] == repr(float(rule_cell(data, sid, s_odds, so, FILE_ORDER)[0]))
            assert np.isclose(float(r[3]), float(b[sid][3]), rtol=1e-12)
            other_bits += r[3] != b[sid][3]
        assert other_bits > 0                                           # the order of the additions is the stored column order
        for n in ("1", "2"):
            assert sorted(run_command(_RuleEngine(), argv + ["--batch-records", n, mixed])[1].splitlines()) == sorted(got.splitlines())


def test_command_libraries_pairing_and_all_motifs(tmp_path):
    from rnascan_amd import pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4, 6), seed=2, ids=["A", "B", "C"])
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4, 6), seed=3, ids=["A", "B", "C"])
    s_odds, q_odds = pssm.load_odds(stp, 0.0, "EHTBLRM", None), pssm.load_odds(seq, 0.0, "GAUC", None)
    rc, text = run_command(_RuleEngine(), ["-p", seq, "-q", stp, "-u", "--all-motifs", fa, st])
    assert rc == 0
    rows = rows_of(text)
    assert [r[0] for r in rows[:3]] == ["A", "B", "C"] and [r[1] for r in rows] == [sid for sid in order for _ in range(3)]
    for r in rows:
        assert r[3] == repr(float(rule_cell(data, r[1], s_odds[r[0]], q_odds[r[0]])[0]))
    assert run_command(_RuleEngine(), ["-p", seq, "-q", stp, "-u", "--all-motifs", "--batch-records", "2", fa, d])[1] == text
    first = run_command(_RuleEngine(), ["-p", seq, "-q", stp, "-u", fa, st])[1]
    assert first.splitlines()[1:] == [ln for ln in text.splitlines()[1:] if ln.startswith("A\t")]
    rc, only = run_command(_RuleEngine(), ["-q", stp, "-u", "--all-motifs", st])
    assert rc == 0 and [r[0] for r in rows_of(only)[:3]] == ["A", "B", "C"]
    for r in rows_of(only):
        assert r[3] == repr(float(rule_cell(data, r[1], s_odds[r[0]])[0]))
    # --pairing positional: the k-th stored column meets the PFM's k-th letter
    rc, pos = run_command(_RuleEngine(), ["-q", stp, "-u", "--pairing", "positional", st])
    assert rc == 0
    for r in rows_of(pos):
        seq_, rows_ = data[r[1]]
        P = np.ascontiguousarray(rows_[:, [STRUCT.index(c) for c in FILE_ORDER]])
        S = np.stack([s_odds["A"][c] for c in STRUCT], axis=1)
        assert r[3] == repr(float(rules.occupancy(P, [0], [len(seq_)], S)[0][0, 0]))


def test_command_errors_open_no_device(tmp_path, capsys):
    """exit 1, nothing on stdout, a message that names the option or the record; engine None: a device would be opened
    (and fail here) if the check came later"""
    fa, d, st, data, order = make_inputs(tmp_path)
    fa2 = tmp_path / "b.fa"
    fa2.write_text(">x\nACGU\n")
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    st5 = write_pfm(tmp_path / "st5.pfm", STRUCT, (5,))
    wide_p = write_pfm(tmp_path / "widep.pfm", "ACGU", (65,))
    wide_q = write_pfm(tmp_path / "wideq.pfm", STRUCT, (65,))
    lib_p = write_pfm(tmp_path / "libp.pfm", "ACGU", (6, 5), ids=["A", "B"])
    lib_q = write_pfm(tmp_path / "libq.pfm", STRUCT, (6, 6), ids=["A", "B"])
    cases = [
        (["-p", seq, "-u", d], ("-p", "-q")),                                        # -p alone with a directory
        (["-p", seq, "-u", st], ("-p", "-q")),
        (["-q", stp, "-u", fa, d], ("-q", "-p")),                                    # -q alone with two inputs
        (["-p", seq, "-u", fa, d], ("-p", "-q")),
        (["-p", seq, "-q", stp, "-u", fa, str(fa2)], ("-p", "-q", "two-FASTA")),     # -p -q with two files
        (["-p", seq, "-q", stp, "-u", fa], ("-p", "-q")),                            # ... with one input
        (["-p", seq, "-q", stp, "-u", d], ("-p", "-q")),
        (["-q", wide_q, "-u", d], ("-q", "PFMSCAN_MAX_M", "65")),
        (["-p", wide_p, "-q", wide_q, "-u", fa, d], ("PFMSCAN_MAX_M", "65")),
        (["-p", seq, "-q", st5, "-u", fa, d], ("-p", "-q", "6", "5")),               # unequal widths of the one pair
        (["-p", lib_p, "-q", lib_q, "-u", "--all-motifs", fa, d], ("B", "5", "6")),  # ... of a pair of two libraries, named
    ]
    for argv, needles in cases:
        rc, text = run_command(None, argv)
        err = capsys.readouterr().err
        assert rc == 1 and text == "", argv
        for needle in needles:
            assert needle in err, (argv, needle, err)


def test_command_input_errors_name_the_record(tmp_path, capsys):
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))

    def fails(argv, *needles, **how):
        rc, text = run_command(_RuleEngine(), argv)
        err = capsys.readouterr().err
        assert rc == 1 and (text == "" or how.get("rows_before")), argv
        for needle in needles:
            assert needle in err, (argv, needle, err)
    base = ["-p", seq, "-q", stp, "-u"]
    text = open(fa).read()
    extra = tmp_path / "extra.fa"
    extra.write_text(text + ">r77\nACGUACGUACGU\n")
    fails(base + [str(extra), d], "r77", "no averaged-structure profile")              # a record without a profile
    fails(base + [str(extra), st], "r77")
    dup = tmp_path / "dup.fa"
    dup.write_text(text + ">r3 again\nACGUACGUACGU\n")
    fails(base + [str(dup), d], "r3", "more than once")                                # a duplicate id
    short = tmp_path / "short.fa"
    short.write_text(text.replace(data["r4"][0], data["r4"][0][:-2]))
    # a length mismatch shows when the record's batch is read: the rows of the batches before it are out by then
    fails(base + [str(short), d], "r4", "10 letters", "12 rows", rows_before=True)
    fails(base + [str(short), st], "r4", "10 letters", "12 rows", rows_before=True)
    less = tmp_path / "less.fa"
    less.write_text("".join(">%s\n%s\n" % (sid, data[sid][0]) for sid in order if sid != "r5"))
    fails(base + [str(less), d], "r5", "no record in the FASTA")                       # a profile without a record
    empty = tmp_path / "empty"
    empty.mkdir()
    fails(["-q", stp, "-u", str(empty)], "No averaged structure files")


def test_command_default_structure_background(tmp_path, capsys):
    """without -u or -B the structure background is background.profile_background of the input: the same bytes as -B of
    that dict, in both modes and both input forms; a cell no background can be computed from ends the run with exit 1"""
    from rnascan_amd import background
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    bg = background.profile_background(_RuleEngine(), st)
    assert sorted(bg) == sorted(STRUCT) and len(set(bg.values())) > 1
    f = tmp_path / "bg.txt"
    f.write_text(repr(bg))
    g = tmp_path / "bg_seq.txt"
    g.write_text(repr(dict(zip("GAUC", (0.3, 0.2, 0.3, 0.2)))))
    for tail in (["-q", stp, st], ["-q", stp, d], ["-p", seq, "-q", stp, "-b", str(g), fa, st], ["-p", seq, "-q", stp, fa, d]):
        rc, text = run_command(_RuleEngine(), tail)
        rc2, want = run_command(_RuleEngine(), ["-B", str(f)] + tail)
        assert rc == 0 and rc2 == 0 and text == want and len(text.splitlines()) == 7
        assert text != run_command(_RuleEngine(), ["-u"] + [a for a in tail if a not in ("-b", str(g))])[1]
    capsys.readouterr()
    write_profile(d, "r3", np.where(np.arange(130)[:, None] == 17, np.nan, data["r3"][1]))
    rc, text = run_command(_RuleEngine(), ["-q", stp, d])
    err = capsys.readouterr().err
    assert rc == 1 and text == "" and "r3" in err and "position 18" in err


def test_command_on_the_histone_example(tmp_path):
    """-p, -q, -u on the shipped histone 3' end with its averaged-structure profile and the SLBP PFMs: every cell is
    finite and positive, and the joint cell is the rule's"""
    from rnascan_amd import fasta, pssm
    d = tmp_path / "avg"
    d.mkdir()
    fa = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
    sid = fasta.open_lazy(fa).ids[0]
    shutil.copy(os.path.join(DATA_DIR, "HIST2H3C_3p_end_structure.txt"), str(d / ("structure.%s.txt" % sid)))
    seq = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
    stp = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")
    cells = {}
    for name, argv in (("joint", ["-p", seq, "-q", stp, "-u", fa, str(d)]), ("struct", ["-q", stp, "-u", str(d)]), ("seq", ["-p", seq, "-u", fa])):
        rc, text = run_command(_RuleEngine(), argv)
        assert rc == 0
        (row,) = rows_of(text)
        x = float(row[3])
        assert row[1] == sid and np.isfinite(x) and x > 0 and int(row[2]) > 0
        cells[name] = row
    letters, prof = fasta.read_profile(str(d / ("structure.%s.txt" % sid)))
    s_odds = next(iter(pssm.load_odds(stp, 0.0, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.0, "GAUC", None).values()))
    rec = list(fasta.open_lazy(fa))[0]
    body = fasta.preprocess_seq(rec.seq, True)
    assert len(body) == prof.shape[0]
    codes = np.array(["ACGU".index(c) if c in "ACGU" else 7 for c in body], dtype=np.uint8)
    S = np.stack([s_odds[c] for c in letters], axis=1)
    occ, win = rules.occupancy(prof, [0], [len(body)], S, codes, q_odds.ratio_table("ACGU"))
    assert cells["joint"][3] == repr(float(occ[0, 0])) and int(cells["joint"][2]) == int(win[0])
    occ, win = rules.occupancy(prof, [0], [len(body)], S)
    assert cells["struct"][3] == repr(float(occ[0, 0])) and int(cells["struct"][2]) == int(win[0]) == len(body) - S.shape[0] + 1
