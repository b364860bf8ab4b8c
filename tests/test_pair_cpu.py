"""Occupancy and expected counts of two code streams on a GPU-less host: the rules (tests/pair_rules.py) against a scalar loop
and against the single-stream rules (the two identities), the bindings, and the two commands' host logic with the rules
standing in for the device.  Every comparison of doubles is on bit patterns."""
import io
import math
import os
import re

import numpy as np
import pytest

import expect_rules as erules
import occupancy_rules as orules
import pair_rules as rules
from conftest import REPO
from test_occupancy_cpu import STRUCT, write_pfm

RNA = "ACGU"


# ---- the rules against a scalar loop -----------------------------------------------------------------------------------
def scalar_tree(values):
    a = [float(x) for x in values]
    if not a:
        return 0.0
    while len(a) > 1:
        nxt = []
        for j in range(0, len(a), 32):
            s = np.float64(a[j])
            for x in a[j + 1:j + 32]:
                s = s + np.float64(x)
            nxt.append(float(s))
        a = nxt
    return a[0]


def scalar_record(codes, codes2, off, length, R, S, mode):
    """the definition of include/pfmscan.h, one window and one product at a time"""
    m = R.shape[0]
    n_win = max(length - m + 1, 0)
    ts, has = [], []
    with np.errstate(all="ignore"):
        for s in range(n_win):
            a = [int(codes[off + s + k]) & 7 for k in range(m)]
            b = [int(codes2[off + s + k]) & 7 for k in range(m)]
            ok = all(x < 4 for x in a) and all(x < 7 for x in b)
            t = np.float64(0.0)
            if ok:
                t = np.float64(R[0][a[0]])
                for k in range(1, m):
                    t = t * np.float64(R[k][a[k]])
                for k in range(m):
                    t = t * np.float64(S[k][b[k]])
            ts.append(float(t))
            has.append(ok)
        occ = scalar_tree(ts)
        if mode == rules.POSTERIOR:
            v = np.float64(1.0) / np.float64(occ) if occ != 0.0 else None
            w = [0.0 if (v is None or not h) else float(np.float64(t) * v) for t, h in zip(ts, has)]
        else:
            w = [t if h else 0.0 for t, h in zip(ts, has)]
        Es, Et = np.zeros((m, 8)), np.zeros((m, 8))
        for k in range(m):
            for c in range(4):
                Es[k, c] = scalar_tree([w[s] if has[s] and (int(codes[off + s + k]) & 7) == c else 0.0 for s in range(n_win)])
            for c in range(7):
                Et[k, c] = scalar_tree([w[s] if has[s] and (int(codes2[off + s + k]) & 7) == c else 0.0 for s in range(n_win)])
    return Es, Et, occ, sum(has)


@pytest.mark.parametrize("mode", [rules.RATIO, rules.POSTERIOR])
def test_rules_against_a_scalar_loop(mode):
    rng = np.random.default_rng(41 + mode)
    for m in (1, 3, 7):
        lengths = [0, m - 1, m, m + 1, m + 30, m + 31, m + 32, 150, 1100][::-1] if m > 1 else [0, 1, 2, 33, 70]
        codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.03, foreign_struct=0.03, case=True)
        R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
        es, et, occ, win = rules.expected(codes, codes2, off, lens, R, S, mode)
        o2, w2 = rules.occupancy(codes, codes2, off, lens, R, S)
        assert rules.same_bits(o2, occ) and np.array_equal(w2, win)
        for r in range(lens.size):
            Es, Et, o, w = scalar_record(codes, codes2, int(off[r]), int(lens[r]), R, S, mode)
            assert rules.same_bits(es[r, 0], Es) and rules.same_bits(et[r, 0], Et) and rules.same_bits(occ[r, 0], o) and win[r] == w
        assert (es[:, :, :, 4:] == 0).all() and (et[:, :, :, 7:] == 0).all()


def test_the_chain_is_letters_first_then_structure_and_never_premultiplied():
    """one window whose three orders of multiplication round differently"""
    R = np.full((2, 8), np.nan)
    S = np.full((2, 8), np.nan)
    R[:, :4] = [[1.1, 0.3, 0.7, 1.9], [0.9, 1.3, 2.3, 0.1]]
    S[:, :7] = [[1.7, 0.3, 0.7, 1.9, 2.1, 0.6, 1.3], [0.9, 1.3, 2.3, 0.1, 1.9, 0.7, 1.1]]
    rng = np.random.default_rng(5)
    found = False
    for _ in range(200):
        a, b = rng.integers(0, 4, size=2), rng.integers(0, 7, size=2)
        codes, codes2 = np.append(a, 7).astype(np.uint8), np.append(b, 7).astype(np.uint8)
        t, has = rules.terms(codes, codes2, 0, 2, R, S)
        chain = ((R[0][a[0]] * R[1][a[1]]) * S[0][b[0]]) * S[1][b[1]]
        pre = (R[0][a[0]] * S[0][b[0]]) * (R[1][a[1]] * S[1][b[1]])
        assert has.all() and t[0] == chain
        found = found or chain != pre
    assert found


# ---- the two identities ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 8, 21])
def test_identities_against_the_single_stream_rules(m):
    rng = np.random.default_rng(50 + m)
    lengths = [int(x) + m - 1 for x in rng.integers(1, 200, size=12)] + [m - 1, 1024 + m - 1, 1100 + m]
    R = np.stack([rules.table(rng, m, 4), rules.table(rng, m, 4)])
    S = np.stack([rules.table(rng, m, 7), rules.table(rng, m, 7)])
    one = np.stack([rules.ones(m)] * 2)
    # S == 1.0, no foreign structure code: the single-stream values on codes
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.01, foreign_struct=0.0, case=True)
    for mode in (rules.RATIO, rules.POSTERIOR):
        es, et, occ, win = rules.expected(codes, codes2, off, lens, R, one, mode)
        e1, o1, w1 = erules.expected(codes, off, lens, R, 4, mode)
        assert rules.same_bits(es, e1) and rules.same_bits(occ, o1) and np.array_equal(win, w1)
    o0, w0 = rules.occupancy(codes, codes2, off, lens, R, one)
    oo, ww = orules.occupancy(codes, off, lens, R, 4)
    assert rules.same_bits(o0, oo) and np.array_equal(w0, ww)
    # R == 1.0, no foreign sequence code: the single-stream values on codes2 with 7 letters
    codes, codes2, off, lens = rules.streams(rng, lengths, foreign_seq=0.0, foreign_struct=0.01, case=True)
    for mode in (rules.RATIO, rules.POSTERIOR):
        es, et, occ, win = rules.expected(codes, codes2, off, lens, one, S, mode)
        e1, o1, w1 = erules.expected(codes2, off, lens, S, 7, mode)
        assert rules.same_bits(et, e1) and rules.same_bits(occ, o1) and np.array_equal(win, w1)


def test_zero_occupancy_and_special_cells():
    rng = np.random.default_rng(6)
    m = 4
    codes, codes2, off, lens = rules.streams(rng, [60])
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    S0 = S.copy()
    S0[1, :7] = 0.0                                                      # every term is +0.0: occ is +0.0
    for mode in (rules.RATIO, rules.POSTERIOR):
        es, et, occ, win = rules.expected_record(codes, codes2, off[0], lens[0], R, S0, mode)
        assert occ == 0 and not np.signbit(occ) and win == 57 and (es == 0).all() and (et == 0).all()
    # 0 x inf across the two chains: the letters reach +inf, the structure holds a zero
    Ri = R.copy()
    Ri[0, :4] = np.inf
    o, w = rules.occupancy(codes, codes2, off, lens, Ri, S0)
    assert np.isnan(o[0, 0]) and w[0] == 57
    # a record that is foreign throughout in one stream
    allbad = np.full(codes2.size, 7, dtype=np.uint8)
    o, w = rules.occupancy(codes, allbad, off, lens, R, S)
    assert o[0, 0] == 0 and not np.signbit(o[0, 0]) and w[0] == 0


def test_chunk_rule():
    assert rules.lds_chunk(12) == 8 and rules.lds_chunk(64) == 2 and rules.lds_chunk(1) > 64
    for m in (1, 2, 8, 12, 21, 64):
        assert rules.lds_chunk(m) >= 1 and rules.lds_chunk(m, 3) <= 3


# ---- bindings --------------------------------------------------------------------------------------------------------
def test_abi_25_exports_the_pair_entry_points():
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    assert _lib.ABI_VERSION >= 25 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION
    for name in ("pfmscan_occupancy_pair_dev", "pfmscan_occupancy_pair_staged", "pfmscan_expect_pair_dev", "pfmscan_expect_pair_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
    for name in ("occupancy_pair_dev", "occupancy_pair_staged", "expect_pair_dev", "expect_pair_staged"):
        assert callable(getattr(_lib.Context, name))
    assert callable(scanner.HipEngine.occupancy_pair) and callable(scanner.HipEngine.expect_pair)
    src = open(os.path.join(REPO, "rnascan_amd", "csrc", "pfmscan_occupancy.hip")).read()
    assert int(re.search(r"OCC_LDS_DOUBLES\s*=\s*(\d+)", src).group(1)) == rules.LDS_DOUBLES and "OCC_PAIR_LETTERS" in src


# ---- the commands with the rules in the device's place -----------------------------------------------------------------
class _RuleEngine(object):
    """HipEngine.occupancy_pair / expect_pair answered by the rules"""

    def occupancy_pair(self, stream, seq_tables, struct_tables):
        return rules.occupancy(stream.codes, stream.codes2, stream.offsets, stream.lengths, seq_tables, struct_tables)

    def expect_pair(self, stream, seq_tables, struct_tables, mode):
        return rules.expected(stream.codes, stream.codes2, stream.offsets, stream.lengths, seq_tables, struct_tables, mode)

    def close(self):
        pass


SEQS = [("r1", "ACGUACGUAAGGCUCUUUUCAGAGCACGU"), ("r2", "acgtnacgtAAAGGCTCTTTTCAGAGCAA"), ("r3", "GG"), ("r4", "ACGGU" * 30), ("r5", "NNNNNNNNNNNN")]
STRUCTS = ["EEEHHHHLLLLHHHHTTTEEEMMMBBBRR", "EEhhhllllhhhTTeemmmBBBrrrEEEE", "EE", "EHHHLLLHHHTTMMB" * 10, "EEEEEEEEEEEE"]


def write_inputs(tmp_path, structs=STRUCTS, ids=None):
    fa, sfa = tmp_path / "seqs.fa", tmp_path / "structs.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s) for i, s in SEQS))
    sfa.write_text("".join(">%s\n%s\n" % (i, s) for i, s in zip(ids or [i for i, _ in SEQS], structs)))
    return str(fa), str(sfa)


def codes_of(text, letters):
    up = text.upper().replace("T", "U") if letters == RNA else text.upper()
    return np.array([letters.index(c) if c in letters else 7 for c in up] + [7], dtype=np.uint8)


def run_occupancy(engine, argv):
    from rnascan_amd import occupancy_pair
    out = io.StringIO()
    rc = occupancy_pair.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def run_expect(engine, argv):
    from rnascan_amd import expect_pair
    return expect_pair.main(argv, engine=engine)


def outputs(prefix):
    return tuple(open(str(prefix) + suffix).read() for suffix in (".expected.seq.txt", ".expected.struct.txt", ".summary.txt"))


def test_occupancy_command_bytes_and_batching(tmp_path):
    from rnascan_amd import fasta, occupancy, pssm
    fa, sfa = write_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6, 4, 6), seed=3)
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4, 6), seed=4)
    base = ["-p", seq, "-q", st, "-u", "-C", "0.01", "--all-motifs", "--struct-format", "letters"]
    rc, text = run_occupancy(_RuleEngine(), base + [fa, sfa])
    assert rc == 0
    lines = text.splitlines()
    assert lines[0].split("\t") == occupancy.COLUMNS and len(lines) == 1 + 5 * 3
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [r[1] for r in rows] == [i for i, _ in SEQS for _ in range(3)] and [r[0] for r in rows[:3]] == ["M0", "M1", "M2"]
    sodds, todds = pssm.load_odds(seq, 0.01, fasta.RNA, None), pssm.load_odds(st, 0.01, fasta.STRUCT, None)
    for r, ((_, s), t) in enumerate(zip(SEQS, STRUCTS)):
        c, c2 = codes_of(s, RNA), codes_of(t, STRUCT)
        for k, mid in enumerate(("M0", "M1", "M2")):
            o, w = rules.occupancy(c, c2, [0], [len(s)], sodds[mid].ratio_table(RNA), todds[mid].ratio_table(STRUCT))
            assert rows[3 * r + k] == [mid, SEQS[r][0], str(int(w[0])), repr(float(o[0, 0])), occupancy.log2_text(o[0, 0])]
    assert rows[6][2:] == ["0", "0.0", "-inf"] and rows[12][2:] == ["0", "0.0", "-inf"]       # r3 is too short, r5 is foreign throughout
    assert rows[3][2] == str(len(SEQS[1][1]) - 5 - 5)                                          # the windows over r2's n have no term
    for n in ("1", "2"):
        assert run_occupancy(_RuleEngine(), base + ["--batch-records", n, fa, sfa])[1] == text
    first = run_occupancy(_RuleEngine(), ["-p", seq, "-q", st, "-u", "-C", "0.01", "--struct-format", "letters", fa, sfa])[1].splitlines()
    assert first[1:] == [ln for ln in lines[1:] if ln.startswith("M0\t")]
    # two single PFMs: the pair is named as the site profiles name it
    one_p, one_q = write_pfm(tmp_path / "a.pfm", RNA, (5,), seed=1), write_pfm(tmp_path / "b.pfm", STRUCT, (5,), seed=2)
    rc, text = run_occupancy(_RuleEngine(), ["-p", one_p, "-q", one_q, "--struct-format", "letters", fa, sfa])
    assert rc == 0 and text.splitlines()[1].startswith("a__b\tr1\t")


def test_expect_command_bytes_batching_and_iterations(tmp_path):
    from rnascan_amd import expect, fasta, pssm
    fa, sfa = write_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6, 4), seed=3)
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=4)
    for weight in ("posterior", "ratio"):
        base = ["-p", seq, "-q", st, "-u", "-C", "0.02", "--all-motifs", "--struct-format", "letters", "--weight", weight]
        assert run_expect(_RuleEngine(), base + ["-o", str(tmp_path / weight), fa, sfa]) == 0
        seq_text, struct_text, summary = outputs(tmp_path / weight)
        lines = summary.splitlines()
        assert lines[0].split("\t") == expect.COLUMNS and [ln.split("\t")[:2] for ln in lines[1:]] == [["M0", "1"], ["M1", "1"]]
        got_seq = dict(pssm.read_multi_pfm(str(tmp_path / weight) + ".expected.seq.txt"))
        got_struct = dict(pssm.read_multi_pfm(str(tmp_path / weight) + ".expected.struct.txt"))
        assert struct_text.splitlines()[1].split("\t") == ["#PO"] + list("BEHLMRT")
        sodds, todds = pssm.load_odds(seq, 0.02, fasta.RNA, None), pssm.load_odds(st, 0.02, fasta.STRUCT, None)
        for mid, m in (("M0", 6), ("M1", 4)):
            per = [rules.expected_record(codes_of(s, RNA), codes_of(t, STRUCT), 0, len(s), sodds[mid].ratio_table(RNA),
                                         todds[mid].ratio_table(STRUCT), expect.MODES[weight]) for (_, s), t in zip(SEQS, STRUCTS)]
            for c, l in enumerate(RNA):
                assert got_seq[mid][l].tolist() == [math.fsum(p[0][k, c] for p in per) for k in range(m)]
            for c, l in enumerate(STRUCT):
                assert got_struct[mid][l].tolist() == [math.fsum(p[1][k, c] for p in per) for k in range(m)]
            row = [ln.split("\t") for ln in lines[1:] if ln.startswith(mid + "\t")][0]
            occ = [p[2] for p in per]
            assert row[2:] == [str(sum(o > 0 for o in occ)), str(sum(o == 0 for o in occ)), str(sum(p[3] for p in per)),
                               repr(round(math.fsum(math.log2(o) for o in occ if o > 0), 3))]
        for n in ("1", "2"):
            assert run_expect(_RuleEngine(), base + ["--batch-records", n, "-o", str(tmp_path / ("b" + n)), fa, sfa]) == 0
            assert outputs(tmp_path / ("b" + n)) == (seq_text, struct_text, summary)
    # --iterations 2 is a run on the outputs of a run, byte for byte -- for a library and for the first pair alone
    for extra in (["--all-motifs"], []):
        base = ["-C", "0.02", "--struct-format", "letters"] + extra
        assert run_expect(_RuleEngine(), ["-p", seq, "-q", st] + base + ["--iterations", "2", "-o", str(tmp_path / "two"), fa, sfa]) == 0
        assert run_expect(_RuleEngine(), ["-p", seq, "-q", st] + base + ["-o", str(tmp_path / "first"), fa, sfa]) == 0
        assert run_expect(_RuleEngine(), ["-p", str(tmp_path / "first") + ".expected.seq.txt", "-q", str(tmp_path / "first") + ".expected.struct.txt"] +
                          base + ["-o", str(tmp_path / "second"), fa, sfa]) == 0
        two, first, second = outputs(tmp_path / "two"), outputs(tmp_path / "first"), outputs(tmp_path / "second")
        assert two[:2] == second[:2] and two[0] != first[0] and two[1] != first[1]
        rows = [ln.split("\t") for ln in two[2].splitlines()[1:]]
        n = len(rows) // 2
        assert [r[1] for r in rows] == ["1"] * n + ["2"] * n
        assert [r[2:] for r in rows[:n]] == [ln.split("\t")[2:] for ln in first[2].splitlines()[1:]]
        assert [r[2:] for r in rows[n:]] == [ln.split("\t")[2:] for ln in second[2].splitlines()[1:]]


def test_errors_before_a_device_is_opened(tmp_path, capsys):
    """exit 1, a message that names the cause, nothing written, and no engine asked for (engine=None would open a device)"""
    fa, sfa = write_inputs(tmp_path)
    seq, st = write_pfm(tmp_path / "seq.pfm", RNA, (6,)), write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    narrow = write_pfm(tmp_path / "narrow.pfm", STRUCT, (5,))
    wide_p, wide_q = write_pfm(tmp_path / "widep.pfm", RNA, (65,)), write_pfm(tmp_path / "wideq.pfm", STRUCT, (65,))
    lib3, lib2 = write_pfm(tmp_path / "lib3.pfm", RNA, (6, 6, 6)), write_pfm(tmp_path / "lib2.pfm", STRUCT, (6, 6))
    with open(lib2) as f:
        renamed = f.read().replace("#M", "#X")                           # two libraries of different size that share no id
    with open(lib2, "w") as f:
        f.write(renamed)
    avg = tmp_path / "avgdir"
    avg.mkdir()
    (tmp_path / "other").mkdir()
    _, swapped = write_inputs(tmp_path / "other", ids=["r1", "r3", "r2", "r4", "r5"])
    (tmp_path / "short").mkdir()
    _, short = write_inputs(tmp_path / "short", structs=STRUCTS[:1] + [STRUCTS[1][:-1]] + STRUCTS[2:])
    (tmp_path / "fewer").mkdir()
    _, fewer = write_inputs(tmp_path / "fewer", structs=STRUCTS[:4])
    prefix = str(tmp_path / "out")
    cases = ((["-p", seq, fa, sfa], ("-p", "-q")), (["-q", st, fa, sfa], ("-p", "-q")),
             (["-p", seq, "-q", st, fa], ("two inputs",)), (["-p", seq, "-q", st, fa, str(avg)], ("averaged-structure",)),
             (["-p", seq, "-q", narrow, fa, sfa], ("seq", "narrow", "6", "5")),
             (["-p", wide_p, "-q", wide_q, fa, sfa], ("PFMSCAN_MAX_M", "65")),
             (["-p", lib3, "-q", lib2, "--all-motifs", fa, sfa], ("cannot be paired",)),
             (["-p", seq, "-q", st, fa, swapped], ("r2", "r3")), (["-p", seq, "-q", st, fa, short], ("r2", "29", "28")),
             (["-p", seq, "-q", st, fa, fewer], ("r5",)))
    for argv, needles in cases:
        rc, text = run_occupancy(None, argv)
        err = capsys.readouterr().err
        assert rc == 1 and text == ""
        for needle in needles:
            assert needle in err, (argv, err)
        rc = run_expect(None, ["-o", prefix] + argv)
        err = capsys.readouterr().err
        assert rc == 1
        for needle in needles:
            assert needle in err, (argv, err)
    assert run_expect(None, ["-o", prefix, "-p", seq, "-q", st, "--iterations", "0", fa, sfa]) == 1
    assert "--iterations" in capsys.readouterr().err
    assert not any(os.path.exists(prefix + s) for s in (".expected.seq.txt", ".expected.struct.txt", ".summary.txt"))


def test_expect_errors_after_the_pass(tmp_path, capsys):
    fa, sfa = write_inputs(tmp_path)
    prefix = str(tmp_path / "out")
    seq, st = write_pfm(tmp_path / "seq.pfm", RNA, (6,)), write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    # a structure background of 0 for a letter the motif has: a ratio is +inf, and r1's occupancy with it
    bg = tmp_path / "bg.txt"
    bg.write_text("{'E': 0.0, 'H': 0.2, 'T': 0.2, 'B': 0.1, 'L': 0.2, 'R': 0.1, 'M': 0.2}")
    assert run_expect(_RuleEngine(), ["-p", seq, "-q", st, "-C", "0.01", "-B", str(bg), "--struct-format", "letters", "-o", prefix, fa, sfa]) == 1
    err = capsys.readouterr().err
    assert "Motif seq__st" in err and "record r1" in err and ("infinite" in err or "not a number" in err)
    # a pair no record contributes to: every window meets a zero on the sequence side
    with open(str(tmp_path / "zero.pfm"), "w") as f:
        f.write("PO\tA\tC\tG\tU\n0\t1\t1\t1\t1\n1\t0\t0\t0\t0\n" + "".join("%d\t1\t1\t1\t1\n" % k for k in range(2, 6)))
    assert run_expect(_RuleEngine(), ["-p", str(tmp_path / "zero.pfm"), "-q", st, "-u", "--struct-format", "letters", "-o", prefix, fa, sfa]) == 1
    err = capsys.readouterr().err
    assert "Motif zero__st" in err and "no record contributes" in err
    assert not any(os.path.exists(prefix + s) for s in (".expected.seq.txt", ".expected.struct.txt", ".summary.txt"))


def test_the_single_stream_commands_still_refuse_two_fastas(tmp_path, capsys):
    from rnascan_amd import expect, occupancy
    fa, sfa = write_inputs(tmp_path)
    seq, st = write_pfm(tmp_path / "seq.pfm", RNA, (6,)), write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    out = io.StringIO()
    assert occupancy.main(["-p", seq, "-q", st, fa, sfa], engine=None, out=out) == 1 and out.getvalue() == ""
    assert "the occupancy of two-FASTA pairs is not supported, run -p and -q one at a time" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        expect.main(["-p", seq, "-q", st, "-o", str(tmp_path / "x"), fa, sfa], engine=None)     # expect takes one input
    capsys.readouterr()
    assert expect.main(["-p", seq, "-q", st, "-o", str(tmp_path / "x"), fa], engine=None) == 1
    assert "not supported" in capsys.readouterr().err
