"""The threshold-free mutagenesis without a device: the rule (tests/mutocc_rules.py) against brute force -- really mutate the
stream and take the posterior site map's ratio cover there --, the bound on Occupancy.Alt, the header and the bindings, and the
command ``python -m rnascan_amd.variant_occupancy`` with the rules in the device's place."""
import io
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import footprint_rules as frules
import mutocc_rules as rules
import occupancy_rules as orules
from conftest import DATA_DIR, REPO
from test_occupancy_cpu import write_pfm

RNA = "ACGU"
HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
SLBP_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
FIXTURE = os.path.join(REPO, "tests", "golden", "variant_occupancy", "hist_slbp_saturate.tsv")
FIXTURE_ARGV = ["-p", SLBP_PFM, "-u", "-C", "0", "--saturate", HIST_FA]


# ---- the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 5, 8])
def test_the_rule_against_really_mutating_the_stream(m):
    rng = np.random.default_rng(100 + m)
    lengths = [0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m, 3 * m + 4, 29]
    codes, off, lens = rules.stream(rng, lengths, 4, foreign=0.04, case=True)
    codes[off[-1] + 5], codes[off[-2] + m] = 5, 4 | 8              # foreign codes inside records, whatever the draw gave
    assert (codes & 8).any()
    R = rules.table(rng, m)
    local, occ, win = rules.mutocc(codes, off, lens, R)
    _, cover, occ2, win2 = frules.footprint(codes, None, off, lens, R, None, frules.RATIO)
    assert rules.same_bits(occ, occ2) and np.array_equal(win, win2)
    inside = np.zeros(codes.size, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
        for i in range(int(n)):
            c = int(codes[o + i]) & 7
            if c >= 4:
                assert np.isnan(local[0, o + i]).all()
                continue
            # the ref column is the unmutated cover, every column the cover of the mutated stream
            assert rules.same_bits(local[0, o + i, c], cover[0, o + i])
            for a in range(4):
                assert rules.same_bits(local[0, o + i, a], rules.cover_with(codes, o, n, R, i, a)), (m, int(n), i, a)
    assert np.isnan(local[0, ~inside]).all()                          # separators: the fill


def test_special_cells_go_where_the_arithmetic_takes_them():
    rng = np.random.default_rng(7)
    m = 4
    codes, off, lens = rules.stream(rng, [12, 3, 30], 4, foreign=0.05)
    for cell in (0.0, np.inf, np.nan):
        R = rules.table(rng, m)
        R[1, 2] = cell
        R[2, 0] = 0.0 if cell == np.inf else R[2, 0]                  # 0 * inf somewhere
        local, _, _ = rules.mutocc(codes, off, lens, R)
        for o, n in zip(off, lens):
            for i in range(int(n)):
                if (int(codes[o + i]) & 7) < 4:
                    for a in range(4):
                        assert rules.same_bits(local[0, o + i, a], rules.cover_with(codes, o, n, R, i, a))


def test_events_are_the_filter_of_the_map():
    rng = np.random.default_rng(11)
    m = 5
    codes, off, lens = rules.stream(rng, [40, 0, 4, 77], 4, foreign=0.03)
    Rs = np.stack([rules.table(rng, m, 4, 0.05, 8.0) for _ in range(2)])
    local, occ, _ = rules.mutocc(codes, off, lens, Rs)
    n_pos = codes.size
    for frac in (0.0, 0.1, 0.5):
        key, alt, ref = rules.events(local, codes, off, lens, occ, frac)
        assert (np.diff(key) > 0).all()
        a, p, q = key & 3, (key >> 2) % n_pos, (key >> 2) // n_pos
        c = codes[p] & 7
        assert (c < 4).all() and (a != c).all()
        assert rules.same_bits(alt, local[q, p, a]) and rules.same_bits(ref, local[q, p, c])
        rec = np.searchsorted(off, p, side="right") - 1
        delta, gain, loss = rules.classify(ref, alt, occ[rec, q], frac)
        assert (gain ^ loss).all()
        # and nothing else passes: count every (q, p, a) by hand
        count = 0
        for qq in range(2):
            for r, (o, n) in enumerate(zip(off, lens)):
                for i in range(int(n)):
                    cc = int(codes[o + i]) & 7
                    for aa in range(4):
                        if cc < 4 and aa != cc:
                            d = local[qq, o + i, aa] - local[qq, o + i, cc]
                            lim = frac * occ[r, qq]
                            count += bool(d > lim or d < -lim)
        assert count == key.size
    assert rules.events(local, codes, off, lens, occ, 0.0)[0].size > rules.events(local, codes, off, lens, occ, 0.5)[0].size
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            rules.events(local, codes, off, lens, occ, bad)


def test_occupancy_alt_is_within_its_bound_of_the_mutated_record():
    rng = np.random.default_rng(13)
    for m, L in ((1, 40), (3, 50), (8, 120), (12, 700)):
        codes, off, lens = rules.stream(rng, [L], 4, foreign=0.01)
        R = rules.table(rng, m, 4, 0.05, 8.0)
        local, occ, _ = rules.mutocc(codes, off, lens, R)
        t, has = orules.terms(codes, 0, L, R, 4)
        T = rules.exact_sum(t)
        n_win = max(L - m + 1, 0)
        for i in rng.choice(L, size=12, replace=False):
            c = int(codes[i]) & 7
            if c >= 4:
                continue
            for a in range(4):
                mutated = codes.copy()
                mutated[i] = a
                t2, _ = orules.terms(mutated, 0, L, R, 4)
                T2 = rules.exact_sum(t2)
                lo, hi = max(i - m + 1, 0), min(i, n_win - 1)
                Lref, Lalt = rules.exact_sum(t[lo:hi + 1]), rules.exact_sum(t2[lo:hi + 1])
                assert T2 == T - Lref + Lalt                                  # the other windows are untouched
                got = rules.occupancy_alt(occ[0, 0], local[0, i, a], local[0, i, c])
                assert abs(Fraction(got) - T2) <= Fraction(rules.occupancy_alt_bound(n_win, m, T, Lref, Lalt, got))
                # it is not the tree of the mutated record, only close to it
                assert abs(got - orules.tree(t2)) <= 2 * rules.occupancy_alt_bound(n_win, m, T, Lref, Lalt, got) + 2 * float(rules.tree_bound(n_win) * T2)


def test_the_header_and_the_bindings_export_the_mutocc_entry_points():
    from rnascan_amd import _lib, build, scanner
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 27
    assert int(re.search(r"#define\s+PFMSCAN_MUTOCC_TILE\s+(\d+)", text).group(1)) == _lib.MUTOCC_TILE
    for name in ("pfmscan_mutocc_dev", "pfmscan_mutocc_staged", "pfmscan_mutocc_events_dev", "pfmscan_mutocc_events_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text)
    assert "pfmscan_mutocc.hip" in build.SOURCES
    assert hasattr(scanner.HipEngine, "mutocc") and hasattr(scanner.HipEngine, "mutocc_events")
    if os.path.exists(build.LIB):
        import ctypes
        lib = ctypes.CDLL(build.LIB)
        for name in ("pfmscan_mutocc_dev", "pfmscan_mutocc_staged", "pfmscan_mutocc_events_dev", "pfmscan_mutocc_events_staged"):
            assert hasattr(lib, name)


# ---- the command with the rules in the device's place ------------------------------------------------------------------
def run_command(engine, argv):
    from rnascan_amd import variant_occupancy
    out = io.StringIO()
    rc = variant_occupancy.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


RECORDS = [("first", "ACGUACGUUUGACCAGUACGGAUUCAGACUUAGGCAUUACGAUCAGG"), ("short", "ACG"), ("foreign", "ACGUNNACGUACNGUACGUAGCUAGCAUCGNACGAUCGAC"),
           ("lower", "acguuagcuagcuagcuagcaucgaucgaucagcuagcuacgacu"), ("last", "GGGAUCCCAUAUAUCGCGCGAUAUAGCGCUAUAGCGC")]


def write_fasta(path, records=RECORDS):
    with open(path, "w") as f:
        for rid, seq in records:
            f.write(">%s some description\n%s\n" % (rid, seq))
    return str(path)


def write_variants(path, rows, header=True):
    with open(path, "w") as f:
        if header:
            f.write("Seq_ID\tPos\tRef\tAlt\n")
        for row in rows:
            f.write("\t".join(str(x) for x in row) + "\n")
    return str(path)


def test_the_reference_example_saturated_is_the_committed_fixture():
    """the reference's example record under the SLBP motif: the window at 213 holds 0.9979 of the occupancy (README, footprint),
    so no position outside 213..230 can remove half of it.  No assertion on the gains."""
    from rnascan_amd import variant_occupancy
    rc, text = run_command(rules.RulesEngine(), FIXTURE_ARGV)
    assert rc == 0
    assert text == open(FIXTURE).read()
    lines = text.splitlines()
    assert lines[0].split("\t") == variant_occupancy.COLUMNS
    rows = [ln.split("\t") for ln in lines[1:]]
    losses = [r for r in rows if r[-1] == "loss"]
    assert losses and all(213 <= int(r[2]) <= 230 for r in losses)
    assert all(r[-1] in ("gain", "loss") for r in rows)
    assert run_command(rules.RulesEngine(), FIXTURE_ARGV + ["--batch-records", "1"])[1] == text


def test_command_saturate_order_columns_and_batching(tmp_path):
    from rnascan_amd import variant_occupancy
    fa = write_fasta(tmp_path / "in.fa")
    pfm = write_pfm(tmp_path / "seq.pfm", RNA, (6, 4, 6))
    base = ["-p", pfm, "-u", "-C", "0.01", "--all-motifs", "--min-change", "0.2", "--saturate"]
    rc, text = run_command(rules.RulesEngine(), base + [fa])
    assert rc == 0
    lines = text.splitlines()
    assert lines[0].split("\t") == variant_occupancy.COLUMNS == ["Motif_ID", "Seq_ID", "Pos", "Ref", "Alt", "Occupancy", "Local.Ref", "Local.Alt",
                                                                  "Delta", "Occupancy.Alt", "Log2.Fold", "Effect"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) > 20 and set(r[-1] for r in rows) == {"gain", "loss"}
    names = [rid for rid, _ in RECORDS]
    motifs = ["M0", "M1", "M2"]
    keys = [(names.index(r[1]), int(r[2]), RNA.index(r[4]), motifs.index(r[0])) for r in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    seqs = dict((rid, s.upper().replace("T", "U")) for rid, s in RECORDS)
    for r in rows:
        occ, ref, alt, delta, occ_alt = (float(x) for x in r[5:10])
        assert seqs[r[1]][int(r[2]) - 1] == r[3] != r[4]
        assert repr(occ) == r[5] and delta == alt - ref
        assert occ_alt == max(math.fsum([occ, alt, -ref]), 0.0)
        assert (r[-1] == "gain") == (delta > 0.2 * occ) and (r[-1] == "loss") == (delta < -(0.2 * occ))
        assert r[10] == ("-inf" if occ_alt == 0.0 else repr(round(math.log2(occ_alt / occ), 3)))
    for n in ("1", "2", "4096"):
        assert run_command(rules.RulesEngine(), base + ["--batch-records", n, fa])[1] == text
    # the first motif alone: its rows of the table above
    rc, one = run_command(rules.RulesEngine(), [x for x in base if x != "--all-motifs"] + [fa])
    assert rc == 0 and one.splitlines()[1:] == [ln for ln in lines[1:] if ln.startswith("M0\t")]
    # a larger share: fewer rows, all of them among the first
    rc, half = run_command(rules.RulesEngine(), ["-p", pfm, "-u", "-C", "0.01", "--all-motifs", "--saturate", fa])
    assert rc == 0 and 0 < len(half.splitlines()) < len(lines)
    assert set(tuple(ln.split("\t")[:5]) for ln in half.splitlines()[1:]) <= set(tuple(r[:5]) for r in rows)


def test_command_variants_file_order_effects_only_and_batching(tmp_path):
    fa = write_fasta(tmp_path / "in.fa")
    pfm = write_pfm(tmp_path / "seq.pfm", RNA, (6, 4))
    sat = run_command(rules.RulesEngine(), ["-p", pfm, "-u", "-C", "0.01", "--all-motifs", "--min-change", "0.2", "--saturate", fa])[1]
    event = dict(((r[0], r[1], r[2], r[4]), r) for r in (ln.split("\t") for ln in sat.splitlines()[1:]))
    picked = [k for k in event if k[0] == "M0"][:3]
    vrows = [("last", 5, "U", "c"), ("first", 1, "A", "G"), ("lower", 3, "g", "T"), ("first", 1, "A", "A"), ("short", 3, "G", "A")]
    seqs = dict((rid, s.upper().replace("T", "U")) for rid, s in RECORDS)
    vrows += [(k[1], int(k[2]), seqs[k[1]][int(k[2]) - 1], k[3]) for k in picked]
    vf = write_variants(tmp_path / "v.tsv", vrows)
    base = ["-p", pfm, "-u", "-C", "0.01", "--all-motifs", "--min-change", "0.2", "--variants", vf]
    rc, text = run_command(rules.RulesEngine(), base + [fa])
    assert rc == 0
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    assert len(rows) == 2 * len(vrows)                                       # one row per variant x motif, file order, then motif order
    for i, v in enumerate(vrows):
        for k, mid in enumerate(("M0", "M1")):
            r = rows[2 * i + k]
            assert r[:5] == [mid, v[0], str(v[1]), v[2].upper().replace("T", "U"), v[3].upper().replace("T", "U")]
            if (mid, v[0], str(v[1]), r[4]) in event:                         # the saturated table's row, byte for byte
                assert r == event[(mid, v[0], str(v[1]), r[4])]
            else:
                assert r[-1] == "none"
    assert rows[6][3] == rows[6][4] == "A" and float(rows[6][8]) == 0.0 and rows[6][-1] == "none"
    assert rows[8][1] == "short" and float(rows[8][5]) == 0.0 and float(rows[8][6]) == 0.0   # shorter than the motif: its rows stay
    assert sum(r[-1] != "none" for r in rows) >= 3
    for n in ("1", "2", "4096"):
        assert run_command(rules.RulesEngine(), base + ["--batch-records", n, fa])[1] == text
    rc, only = run_command(rules.RulesEngine(), base + ["--effects-only", fa])
    assert rc == 0 and only.splitlines() == [text.splitlines()[0]] + [ln for ln in text.splitlines()[1:] if not ln.endswith("\tnone")]

    class Counting(rules.RulesEngine):
        seen = []

        def mutocc(self, stream, ratio_tables):
            self.seen.append(len(stream.offsets))
            return rules.RulesEngine.mutocc(self, stream, ratio_tables)

    # only the records the file names are packed
    write_variants(tmp_path / "two.tsv", [("last", 5, "U", "C"), ("first", 1, "A", "G")], header=False)
    rc, _ = run_command(Counting(), ["-p", pfm, "-u", "--variants", str(tmp_path / "two.tsv"), fa])
    assert rc == 0 and Counting.seen == [2]


def test_a_record_of_occupancy_zero_keeps_its_rows(tmp_path):
    fa = write_fasta(tmp_path / "in.fa", [("zero", "AAAAAAAAAAAA"), ("other", "ACGUACGUACGU")])
    pfm = tmp_path / "seq.pfm"
    pfm.write_text("PO\tA\tC\tG\tU\n0\t0\t0.5\t0.25\t0.25\n1\t0.25\t0.25\t0.25\t0.25\n2\t0.25\t0.25\t0.25\t0.25\n")
    rc, text = run_command(rules.RulesEngine(), ["-p", str(pfm), "-u", "--saturate", fa])
    rows = [ln.split("\t") for ln in text.splitlines()[1:] if ln.split("\t")[1] == "zero"]
    assert rc == 0 and rows and all(float(r[5]) == 0.0 and r[-1] == "gain" and r[10] == "inf" and float(r[8]) > 0 for r in rows)
    assert all(r[3] == "A" for r in rows)


def test_every_exit_1_path(tmp_path, capsys):
    fa = write_fasta(tmp_path / "in.fa")
    pfm = write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    wide = write_pfm(tmp_path / "wide.pfm", RNA, (65,))
    ok = write_variants(tmp_path / "ok.tsv", [("first", 1, "A", "G")])
    for argv in (["-p", pfm, fa], ["-p", pfm, "--saturate", "--variants", ok, fa], ["-p", pfm, "--saturate", "--min-change", "-1", fa],
                 ["-p", pfm, "--saturate", "--min-change", "nan", fa], ["-p", pfm, "--saturate", "--batch-records", "0", fa],
                 ["-p", pfm, "-u", "-b", "bg.txt", "--saturate", fa], ["--saturate", fa]):
        with pytest.raises(SystemExit) as e:                                 # the parser's own refusals
            run_command(None, argv)
        assert e.value.code == 2
    capsys.readouterr()
    cases = [
        (["-p", pfm, "-u", "--saturate", str(tmp_path)], ("averaged-structure", "refolding")),
        (["-p", pfm, "-u", "--saturate", fa, fa], ("one input",)),
        (["-p", wide, "-u", "--saturate", fa], ("PFMSCAN_MAX_M", "65")),
        (["-p", pfm, "-u", "--saturate", str(tmp_path / "missing.fa")], ("missing.fa",)),
        (["-p", pfm, "-u", "--variants", str(tmp_path / "missing.tsv"), fa], ("missing.tsv",)),
        (["-p", pfm, "-u", "--variants", write_variants(tmp_path / "a.tsv", [("nobody", 1, "A", "G")]), fa], ("line 2", "unknown Seq_ID")),
        (["-p", pfm, "-u", "--variants", write_variants(tmp_path / "b.tsv", [("short", 4, "A", "G")]), fa], ("line 2", "outside record short")),
        (["-p", pfm, "-u", "--variants", write_variants(tmp_path / "c.tsv", [("first", 1, "A", "G"), ("first", 2, "A", "G")]), fa], ("line 3", "Ref A is not the letter")),
        (["-p", pfm, "-u", "--variants", write_variants(tmp_path / "d.tsv", [("foreign", 5, "A", "G")]), fa], ("not a nucleotide",)),
        (["-p", pfm, "-u", "--variants", write_variants(tmp_path / "e.tsv", [("first", 1, "A", "GG")]), fa], ("indels are not supported",)),
        (["-p", pfm, "-u", "--variants", write_variants(tmp_path / "f.tsv", [("first", "x", "A", "G")]), fa], ("not an integer",)),
    ]
    for argv, needles in cases:
        rc, text = run_command(rules.RulesEngine(), argv)
        err = capsys.readouterr().err
        assert rc == 1 and text == "", argv
        for needle in needles:
            assert needle in err, (argv, err)
    # an infinite occupancy names the motif and the record, in both modes and at any batch size; nothing is written
    bg = tmp_path / "bg.txt"
    bg.write_text("{'A': 0.0, 'C': 0.3, 'G': 0.3, 'U': 0.4}")
    for extra in (["--saturate"], ["--saturate", "--batch-records", "1"], ["--variants", ok], ["--variants", ok, "--batch-records", "1"]):
        rc, text = run_command(rules.RulesEngine(), ["-p", pfm, "-C", "0.01", "-b", str(bg)] + extra + [fa])
        err = capsys.readouterr().err
        assert rc == 1 and text == ""
        assert "Motif seq" in err and "record first" in err and ("infinite" in err or "not a number" in err)
