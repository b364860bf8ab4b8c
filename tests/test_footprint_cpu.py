"""The posterior site map without a device: the rules (tests/footprint_rules.py) against their own bounds and identities, the
known SLBP site of the reference's example record, and the host logic of `python -m rnascan_amd.footprint` with the rules in the
device's place."""
import io
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import expect_rules as erules
import footprint_rules as rules
import occupancy_rules as orules
import pair_rules as prules
from conftest import DATA_DIR, REPO
from test_occupancy_cpu import write_pfm
from test_pair_cpu import SEQS, STRUCTS, write_inputs

RNA = "ACGU"
STRUCT = "EHLMRTB"
HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
SLBP_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
MODES = (rules.RATIO, rules.POSTERIOR)


def ladder(m):
    return [0, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1, 2 * m, 300, 1100]


# ---- the rules -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 12, 33, 64])
def test_bounds_and_identities_on_the_ladder(m):
    rng = np.random.default_rng(100 + m)
    lengths = [max(x, 0) for x in ladder(m)]
    codes, codes2, off, lens = prules.streams(rng, lengths, foreign_seq=0.01, foreign_struct=0.01, case=True)
    R, S = rules.table(rng, m, 4, 0.6, 1.7), rules.table(rng, m, 7, 0.6, 1.7)
    for Rq, Sq in ((R, None), (None, S), (R, S)):
        for mode in MODES:
            start, cover, occ, win = rules.footprint(codes, codes2, off, lens, Rq, Sq, mode)
            assert not np.signbit(start).any() and not np.signbit(cover).any() and np.isfinite(cover).all()
            for r, (o, n) in enumerate(zip(off, lens)):
                o, n = int(o), int(n)
                n_win = max(n - m + 1, 0)
                s, c = start[0, o:o + n], cover[0, o:o + n]
                assert (s[n_win:] == 0).all() and s[n_win:].size == min(m - 1, n)
                assert start[0, o + n] == 0 and cover[0, o + n] == 0       # the separator: in no record
                if n_win == 0:
                    assert (c == 0).all() and occ[r, 0] == 0
                    continue
                # the weights are the expected counts' weights, the occupancy the occupancy's
                t, has = rules.record_terms(codes, codes2, o, n, Rq, Sq)
                assert occ[r, 0] == orules.tree(t) and win[r] == has.sum()
                assert rules.same_bits(s[:n_win], erules.weights(t, has, occ[r, 0], mode))
                # the first and the last position lie under one window each
                assert c[0] == s[0] and c[n - 1] == s[n_win - 1]
                total, covered = rules.exact_sum(s), rules.exact_sum(c)
                assert abs(covered - m * total) <= Fraction(rules.total_bound(m)) * m * total
                if mode == rules.POSTERIOR and occ[r, 0] > 0:
                    assert c.max() <= rules.cover_bound(n_win, m)
                    if m > 1 and n_win > m:
                        assert c.max() > s.max() or (s > 0).sum() <= 1   # a cover is a sum, not the greatest weight


def test_a_lone_window_is_copied():
    rng = np.random.default_rng(3)
    for m in (1, 5, 64):
        codes, off, lens = rules.stream(rng, [m], 4)
        R = rules.table(rng, m, 4)
        for mode in MODES:
            start, cover, occ, win = rules.footprint(codes, None, off, lens, R, None, mode)
            w0 = start[0, 0]
            assert w0 > 0 and win[0] == 1 and (start[0, 1:] == 0).all()
            assert rules.same_bits(cover[0, :m], np.full(m, w0))           # every position under the one window: its weight, bit for bit
            assert w0 == (occ[0, 0] if mode == rules.RATIO else occ[0, 0] * (1.0 / occ[0, 0]))


def test_cover_is_m_additions_in_ascending_order_not_a_sliding_update():
    """three weights whose sum depends on the order: the rule adds them from the lowest start up, position by position"""
    w = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 1.0])
    start, cover = rules.maps_of_weights(w, 6, 3)
    assert cover[2] == (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0               # ascending: both small terms are lost one by one
    assert cover[3] == (2.0 ** -53 + 2.0 ** -53) + 1.0 == 1.0 + 2.0 ** -52   # ascending from the small ones: they survive
    assert cover[0] == 1.0 and cover[5] == 1.0 and cover[4] == 2.0 ** -53 + 1.0
    assert list(start) == [1.0, 2.0 ** -53, 2.0 ** -53, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("nl", [4, 7])
def test_start_map_by_letter_is_the_expected_counts(nl):
    rng = np.random.default_rng(7 + nl)
    m = 5
    codes, off, lens = rules.stream(rng, [0, 4, 5, 6, 40, 200, 1100], nl, foreign=0.01, case=nl == 7)
    T = rules.table(rng, m, nl)
    for mode in MODES:
        if nl == 4:
            start, _, occ, win = rules.footprint(codes, None, off, lens, T, None, mode)
        else:
            start, _, occ, win = rules.footprint(None, codes, off, lens, None, T, mode)
        E, occ_e, win_e = erules.expected(codes, off, lens, T, nl, mode)
        assert rules.same_bits(occ, occ_e) and np.array_equal(win, win_e)
        for r, (o, n) in enumerate(zip(off, lens)):
            _, has = orules.terms(codes, o, n, T, nl)
            want = np.zeros((m, 8))
            if has.size:
                want[:, :nl] = erules.tree_rows(rules.by_letter(start[0, o:o + n], codes[o:o + n], has, m, nl)).reshape(m, nl)
            assert rules.same_bits(want, E[r, 0])


def test_pair_identities_and_special_cells():
    rng = np.random.default_rng(11)
    m = 7
    codes, codes2, off, lens = prules.streams(rng, [3, 50, 400], case=True)
    R, S = rules.table(rng, m, 4), rules.table(rng, m, 7)
    for mode in MODES:
        a = rules.footprint(codes, codes2, off, lens, R, prules.ones(m), mode)
        b = rules.footprint(codes, codes2, off, lens, R, None, mode)
        assert all(rules.same_bits(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[3], b[3])
        a = rules.footprint(codes, codes2, off, lens, prules.ones(m), S, mode)
        b = rules.footprint(codes, codes2, off, lens, None, S, mode)
        assert all(rules.same_bits(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[3], b[3])
        Z = R.copy()
        Z[0, :4] = 0.0
        start, cover, occ, _ = rules.footprint(codes, None, off, lens, Z, None, mode)
        assert (occ == 0).all() and (start == 0).all() and (cover == 0).all() and not np.signbit(cover).any()
        N = R.copy()
        N[3, 1] = np.nan
        _, cover, occ, _ = rules.footprint(codes, None, off, lens, N, None, mode)
        assert np.isnan(occ[2, 0]) and np.isnan(cover).any()


def test_the_header_and_the_bindings_export_the_footprint_entry_points():
    from rnascan_amd import _lib, build
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+PFMSCAN_FOOTPRINT_SLOTS\s+(\d+)", text).group(1)) == _lib.FOOTPRINT_SLOTS
    for name in ("pfmscan_footprint_dev", "pfmscan_footprint_staged", "pfmscan_footprint_events_dev", "pfmscan_footprint_events_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text)
    assert "pfmscan_footprint.hip" in build.SOURCES
    from rnascan_amd import scanner
    assert hasattr(scanner.HipEngine, "footprint") and hasattr(scanner.HipEngine, "footprint_events")


# ---- the command with the rules in the device's place ------------------------------------------------------------------
def run_command(engine, argv):
    from rnascan_amd import footprint
    out = io.StringIO()
    rc = footprint.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def test_the_known_slbp_site_without_a_threshold(golden):
    """the reference's example record under the SLBP motif: the positions with cover > 0.5 are the 18-wide window at start 213,
    which is the arg-max window of the golden thresholded scan"""
    from rnascan_amd import fasta, footprint, pack, pssm
    rc, text = run_command(rules.RulesEngine(), ["-p", SLBP_PFM, "-u", "-C", "0", HIST_FA])
    assert rc == 0
    lines = text.splitlines()
    assert lines[0].split("\t") == footprint.COLUMNS and len(lines) == 2
    row = lines[1].split("\t")
    assert row[2:4] == ["213", "230"] and 213 <= int(row[4]) <= 230
    # the covers by the rules, not retyped
    odds = pssm.load_odds(SLBP_PFM, 0.0, fasta.RNA, None)
    mid = next(iter(odds))
    R = odds[mid].ratio_table(pack.RNA_LETTERS)
    seq = "".join(ln.strip() for ln in open(HIST_FA).read().splitlines()[1:]).upper().replace("T", "U")
    codes = np.array([pack.RNA_LETTERS.index(c) if c in pack.RNA_LETTERS else 7 for c in seq] + [7], dtype=np.uint8)
    start, cover, occ, _ = rules.footprint(codes, None, [0], [len(seq)], R, None, rules.POSTERIOR)
    assert R.shape[0] == 18 and 19645.3 < occ[0, 0] < 19645.4
    assert list(np.flatnonzero(cover[0] > 0.5) + 1) == list(range(213, 231))
    assert int(np.argmax(start[0])) + 1 == 213 and 0.9979 < start[0, 212] < 0.998
    assert row[0] == mid and float(row[5]) == cover[0].max() and int(row[4]) == int(np.argmax(cover[0])) + 1
    assert float(row[6]) == start[0, 212]                                   # one window lies wholly inside the region
    case = next(c for c in golden["pwm"] if c["name"] == "hist_slbp_pc0_uniform")
    assert case["sequence"] == seq and int(np.argmax(np.asarray(case["scores"]))) + 1 == 213


def test_regions_merge_peak_and_mass():
    from rnascan_amd import footprint
    m = 4
    pos = np.array([0, 1, 2, 7, 8, 9, 10, 11, 19])
    cover = np.array([0.6, 0.9, 0.9, 0.7, 0.8, 0.95, 0.95, 0.6, 0.7])
    start = np.array([0.5, 0.25, 0.125, 0.1, 0.2, 0.3, 0.4, 0.5, 0.7])
    got = footprint.regions(pos, cover, start, m)
    # a region at the record's first position, shorter than m: no window lies inside it
    assert got[0] == (0, 2, 1, 0.9, 0.0)
    # the lowest position of greatest cover; the windows that start in [7, 11 - 4 + 1] = 7, 8
    assert got[1] == (7, 11, 9, 0.95, math.fsum([0.1, 0.2]))
    assert got[2] == (19, 19, 19, 0.7, 0.0)
    assert footprint.regions(pos[:0], cover[:0], start[:0], m) == []
    assert footprint.regions(np.array([3]), np.array([0.9]), np.array([0.8]), 1) == [(3, 3, 3, 0.9, 0.8)]


def planted(tmp_path):
    """records with the SLBP site planted at the first position, at the last, twice, and not at all"""
    site = "AAAGGCUCUUUUCAGAGC"
    rng = np.random.default_rng(5)
    noise = lambda n: "".join("ACGU"[c] for c in rng.integers(0, 4, size=n))
    recs = [("first", site + noise(60)), ("last", noise(70) + site), ("twice", noise(30) + site + noise(40) + site + noise(25)), ("none", noise(90)),
            ("short", "ACG"), ("foreign", "N" * 40), ("lower", noise(20).lower() + site.lower().replace("u", "t") + noise(20))]
    fa = tmp_path / "planted.fa"
    fa.write_text("".join(">%s\n%s\n" % r for r in recs))
    return str(fa), recs, site


def test_command_regions_positions_and_batching(tmp_path):
    from rnascan_amd import footprint
    fa, recs, site = planted(tmp_path)
    base = ["-p", SLBP_PFM, "-u", "-C", "0.01"]
    rc, text = run_command(rules.RulesEngine(), base + [fa])
    assert rc == 0
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    by_rec = {}
    for r in rows:
        by_rec.setdefault(r[1], []).append(r)
    m = len(site)
    assert by_rec["first"][0][2] == "1" and by_rec["last"][-1][3] == str(len(recs[1][1]))   # regions at a record's first and last position
    # one site per record is the model: `none` may well have a row (its best window), records with occupancy 0 have none
    assert "short" not in by_rec and "foreign" not in by_rec
    assert [r[1] for r in rows] == sorted([r[1] for r in rows], key=[i for i, _ in recs].index)   # record order
    # two sites of equal weight share the posterior, about a half each: neither passes 0.6, both pass 0.25
    rc, high = run_command(rules.RulesEngine(), base + ["--min-cover", "0.6", fa])
    assert rc == 0 and {ln.split("\t")[1] for ln in high.splitlines()[1:]} == {"first", "last", "none", "lower"}
    rc, low = run_command(rules.RulesEngine(), base + ["--min-cover", "0.25", fa])
    twice = [ln.split("\t") for ln in low.splitlines()[1:] if ln.split("\t")[1] == "twice"]
    assert rc == 0 and len(twice) == 2 and int(twice[0][3]) < int(twice[1][2])
    assert [int(twice[0][2]), int(twice[1][2])] == [31, 31 + m + 40]
    for r in rows + twice:
        for x in r[5:]:
            assert repr(float(x)) == x
        assert int(r[2]) <= int(r[4]) <= int(r[3])
    # --positions: the same events, one row each
    rc, ptext = run_command(rules.RulesEngine(), base + ["--positions", fa])
    prow = [ln.split("\t") for ln in ptext.splitlines()[1:]]
    assert rc == 0 and ptext.splitlines()[0].split("\t") == footprint.POSITION_COLUMNS
    assert len(prow) == sum(int(r[3]) - int(r[2]) + 1 for r in rows)
    for r in rows:
        mine = [p for p in prow if p[1] == r[1] and int(r[2]) <= int(p[2]) <= int(r[3])]
        covers = [float(p[4]) for p in mine]
        assert float(r[5]) == max(covers) and int(r[4]) == int(mine[covers.index(max(covers))][2])
        inside = [float(p[3]) for p in mine if int(p[2]) <= int(r[3]) - m + 1]
        assert float(r[6]) == (math.fsum(inside) if inside else 0.0)
    # the bytes do not depend on --batch-records
    for n in ("1", "2", "7"):
        assert run_command(rules.RulesEngine(), base + ["--batch-records", n, fa])[1] == text
        assert run_command(rules.RulesEngine(), base + ["--positions", "--batch-records", n, fa])[1] == ptext
    # ratio weights need their threshold; with one the rows are those of the likelihood ratios
    rc, rtext = run_command(rules.RulesEngine(), base + ["--weight", "ratio", "--min-cover", "1000", fa])
    assert rc == 0 and {ln.split("\t")[1] for ln in rtext.splitlines()[1:]} >= {"first", "last", "twice", "lower"}


def test_command_motif_order_pairs_and_structure(tmp_path):
    fa, sfa = write_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6, 4, 6), seed=3)
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4, 6), seed=4)
    for argv in (["-p", seq, "-u", fa], ["-q", st, "-u", sfa], ["-p", seq, "-q", st, "-u", fa, sfa]):
        rc, text = run_command(rules.RulesEngine(), argv + ["--all-motifs", "--min-cover", "0.05", "--positions"])
        assert rc == 0
        rows = [ln.split("\t") for ln in text.splitlines()[1:]]
        assert len(rows) > 10
        ids = [i for i, _ in SEQS]
        keys = [(ids.index(r[1]), int(r[0].split("M")[1][0]), int(r[2])) for r in rows]
        assert keys == sorted(keys)                                        # record order, then the file's motif order, then position
        assert len({k[1] for k in keys}) == 3
        for n in ("1", "3"):
            assert run_command(rules.RulesEngine(), argv + ["--all-motifs", "--min-cover", "0.05", "--positions", "--batch-records", n])[1] == text
        first = run_command(rules.RulesEngine(), argv + ["--min-cover", "0.05", "--positions"])[1].splitlines()
        assert first[1:] == [ln for ln, k in zip(text.splitlines()[1:], keys) if k[1] == 0]


def test_option_errors(tmp_path, capsys):
    fa, sfa = write_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    st5 = write_pfm(tmp_path / "st5.pfm", STRUCT, (5,))
    wide = write_pfm(tmp_path / "wide.pfm", RNA, (65,))
    for argv in (["-p", seq, "--weight", "ratio", fa], ["-p", seq, "--min-cover", "nan", fa], ["-p", seq, "--batch-records", "0", fa],
                 ["-p", seq, "-u", "-b", "bg.txt", fa]):
        with pytest.raises(SystemExit) as e:                               # the parser's own refusals
            run_command(None, argv)
        assert e.value.code == 2
    assert "--min-cover" in capsys.readouterr().err
    for argv, needles in (([fa], ("-p", "-q")), (["-p", seq, fa, sfa], ("-p", "one input")), (["-p", seq, "-q", st, fa], ("two inputs",)),
                          (["-p", wide, "-u", fa], ("-p", "PFMSCAN_MAX_M", "65")), (["-p", seq, "-q", st5, "-u", fa, sfa], ("share no window",)),
                          (["-p", seq, "-u", str(tmp_path)], ("averaged-structure",))):
        rc, text = run_command(None, argv)
        err = capsys.readouterr().err
        assert rc == 1 and text == ""
        for needle in needles:
            assert needle in err
    # two FASTA files that do not match are refused as occupancy_pair refuses them
    _, bad = write_inputs(tmp_path, structs=STRUCTS[:1] + [STRUCTS[1][:-1]] + STRUCTS[2:])
    rc, text = run_command(rules.RulesEngine(), ["-p", seq, "-q", st, "-u", fa, bad])
    assert rc == 1 and text == "" and "r2" in capsys.readouterr().err


def test_nan_occupancy_exits_and_zero_occupancy_is_counted(tmp_path, capsys):
    fa, recs, site = planted(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    bg = tmp_path / "bg.txt"
    bg.write_text("{'A': 0.0, 'C': 0.3, 'G': 0.3, 'U': 0.4}")              # a ratio is +inf, and the first record's occupancy with it
    for extra in ([], ["--batch-records", "1"], ["--positions"]):
        rc, text = run_command(rules.RulesEngine(), ["-p", seq, "-C", "0.01", "-b", str(bg), fa] + extra)
        err = capsys.readouterr().err
        assert rc == 1 and text == ""                                      # nothing is written
        assert "Motif seq" in err and "record first" in err and ("infinite" in err or "not a number" in err)
    rc, text = run_command(rules.RulesEngine(), ["-p", SLBP_PFM, "-u", "-C", "0.01", fa])
    err = capsys.readouterr().err
    assert rc == 0 and "2 record x motif pairs have occupancy 0" in err    # `short` and `foreign`
    # a negative threshold reports every position of a record, but never one of a record whose occupancy is 0
    rc, text = run_command(rules.RulesEngine(), ["-p", SLBP_PFM, "-u", "-C", "0.01", "--weight", "ratio", "--min-cover", "-1", fa])
    names = [ln.split("\t")[1] for ln in text.splitlines()[1:]]
    assert rc == 0 and "short" not in names and "foreign" not in names and "none" in names
    row = [ln.split("\t") for ln in text.splitlines()[1:] if ln.split("\t")[1] == "none"]
    assert len(row) == 1 and row[0][2:4] == ["1", "90"]
