"""The posterior site map on averaged-structure profiles without a device: the rules (tests/footprint_profile_rules.py) against
the bounds and the letter rules they must reduce to, the known SLBP site of the reference's example record, the bindings, and
the host logic of `python -m rnascan_amd.footprint_profile` with the rules in the device's place."""
import io
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

import expect_rules as erules
import footprint_profile_rules as rules
import footprint_rules as frules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import pair_rules
from conftest import DATA_DIR, REPO
from test_occupancy_profile_cpu import FILE_ORDER, STRUCT, make_inputs, write_pfm, write_profile

MODES = (rules.RATIO, rules.POSTERIOR)
HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
HIST_PROFILE = os.path.join(DATA_DIR, "HIST2H3C_3p_end_structure.txt")
SLBP_SEQ = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
SLBP_STRUCT = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")


# ---- bindings ----------------------------------------------------------------------------------------------------------
def test_the_header_and_the_bindings_export_the_four_entry_points():
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == L.pfmscan_abi_version() == 27
    for name in ("pfmscan_footprint_profile_dev", "pfmscan_footprint_profile_staged", "pfmscan_footprint_profile_events_dev",
                 "pfmscan_footprint_profile_events_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
        assert callable(getattr(_lib.Context, name[len("pfmscan_"):]))
    assert int(re.search(r"#define\s+PFMSCAN_FOOTPRINT_PROFILE_SLOTS\s+(\d+)", text).group(1)) == _lib.FOOTPRINT_PROFILE_SLOTS
    assert _lib.FOOTPRINT_PROFILE_SLOTS % 256 == 0 and _lib.FOOTPRINT_PROFILE_SLOTS > _lib.MAX_M - 1
    assert "pfmscan_footprint_profile.hip" in build.SOURCES and "pfmscan_fp.hpp" in build.HEADERS and "pfmscan_fp_plan.hpp" in build.HEADERS
    assert callable(scanner.HipEngine.footprint_profile) and callable(scanner.HipEngine.footprint_profile_events)


# ---- the rules ---------------------------------------------------------------------------------------------------------
def ladder(m):
    return [0, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1, 2 * m, 300, 1100]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [1, 2, 12, 33, 64])
def test_bounds_and_identities_on_the_ladder(m, dtype):
    rng = np.random.default_rng(200 + m)
    codes, profile, off, lens = prules.stream(rng, [max(x, 0) for x in ladder(m)], dtype, foreign=0.01)
    S, R = prules.struct_table(rng, m, 0.6, 1.7), orules.table(rng, m, 4, 0.6, 1.7)
    for Rq in (None, R):
        for mode in MODES:
            start, cover, occ, win = rules.footprint(profile, off, lens, S, codes, Rq, mode)
            assert not np.signbit(start).any() and not np.signbit(cover).any() and np.isfinite(cover).all()   # non-negative rows
            for r, (o, n) in enumerate(zip(off, lens)):
                o, n = int(o), int(n)
                n_win = max(n - m + 1, 0)
                s, c = start[0, o:o + n], cover[0, o:o + n]
                assert (s[n_win:] == 0).all() and s[n_win:].size == min(m - 1, n)
                assert start[0, o + n] == 0 and cover[0, o + n] == 0       # the separator (NaN rows): in no record
                if n_win == 0:
                    assert (c == 0).all() and occ[r, 0] == 0
                    continue
                # term, occupancy and weight are the family's
                t, has = prules.terms(profile, o, n, S, codes, Rq)
                assert occ[r, 0] == orules.tree(t) and win[r] == has.sum()
                assert rules.same_bits(s[:n_win], erules.weights(t, has, occ[r, 0], mode))
                assert c[0] == s[0] and c[n - 1] == s[n_win - 1]           # the first and the last position lie under one window
                total, covered = rules.exact_sum(s), rules.exact_sum(c)
                assert abs(covered - m * total) <= Fraction(rules.total_bound(m)) * m * total
                if mode == rules.POSTERIOR and occ[r, 0] > 0:
                    assert c.max() <= rules.cover_bound(n_win, m)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 5, 12])
def test_one_hot_rows_reduce_to_the_letter_rules(m, mode):
    """rows with a single 1 and finite tables: the marginal is the table cell exactly, so structure only is the footprint of the
    structure table over the letter codes and joint is the pair rule over (codes, letter codes), bit for bit"""
    rng = np.random.default_rng(300 + m)
    codes, letters, off, lens = pair_rules.streams(rng, [0, m - 1, m, 2 * m + 3, 150, 400], foreign_seq=0.01, foreign_struct=0.0)
    S = prules.struct_table(rng, m)
    S8 = np.full((m, 8), np.nan)
    S8[:, :7] = S
    R = orules.table(rng, m, 4)
    for dtype in (np.float32, np.float64):
        profile = prules.one_hot(letters, dtype)
        got = rules.footprint(profile, off, lens, S, None, None, mode)
        want = frules.footprint(None, letters, off, lens, None, S8, mode)
        assert all(rules.same_bits(g, w) for g, w in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3])
        got = rules.footprint(profile, off, lens, S, codes, R, mode)
        want = frules.footprint(codes, letters, off, lens, R, S8, mode)
        assert all(rules.same_bits(g, w) for g, w in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3])


def test_a_negative_occupancy_keeps_its_weights():
    """negative cells are legal: with an odd width every term of an all-negative record is negative, so is the occupancy and so
    is v = 1 / occ -- and the weights are t * v, not zero.  This states what the RULES say of such a record (the command's
    test below prints it); that the kernel decides on occ == 0.0 and not on the sign of v is pinned on the device, by
    test_special_cells of tests/test_gpu_footprint_profile.py"""
    rng = np.random.default_rng(7)
    m = 5
    codes, profile, off, lens = prules.stream(rng, [60], np.float64)
    profile[:60] *= -1
    S = prules.struct_table(rng, m)
    start, cover, occ, _ = rules.footprint(profile, off, lens, S, None, None, rules.POSTERIOR)
    assert occ[0, 0] < 0 and (start[0, :56] > 0).all() and 0.999 < start[0].sum() < 1.001 and cover[0].max() > 0


# ---- the command with the rules in the device's place ------------------------------------------------------------------
def run_command(engine, argv):
    from rnascan_amd import footprint_profile
    out = io.StringIO()
    rc = footprint_profile.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def rule_lines(data, sid, mid, struct_odds, seq_odds, mode, thr, positions, cols=FILE_ORDER, dtype=np.float64):
    """the lines of one record under one motif as the rules and footprint.format_rows give them, the rows stored in column order
    ``cols`` -> (lines, occupancy)"""
    from rnascan_amd import footprint
    seq, rows = data[sid]
    profile = np.ascontiguousarray(rows[:, [STRUCT.index(c) for c in cols]]).astype(dtype)
    S = np.stack([struct_odds[c] for c in cols], axis=1)
    codes = np.array(["ACGU".index(c) if c in "ACGU" else 7 for c in seq], dtype=np.uint8)
    R = None if seq_odds is None else seq_odds.ratio_table("ACGU")
    start, cover, occ, _ = rules.footprint(profile, [0], [len(seq)], S, codes, R, mode)
    key, c, w = rules.events(start, cover, [0], [len(seq)], thr)
    if occ[0, 0] == 0.0:
        return [], 0.0
    return footprint.format_rows(mid, sid, key, c, w, S.shape[0], positions), occ[0, 0]


def dir_order(d):
    """the record order of a directory (or store) on its own: the one every command of the family walks it in"""
    from rnascan_amd import sites
    return list(sites._Profiles(d, np.float64).ids)


def hist_dir(tmp_path):
    d = tmp_path / "hist"
    d.mkdir()
    sid = open(HIST_FA).readline()[1:].split()[0]
    shutil.copyfile(HIST_PROFILE, d / ("structure.%s.txt" % sid))
    return str(d), sid


def test_the_known_slbp_site_without_a_threshold(tmp_path, golden):
    """the reference's example record and its averaged-structure profile: the positions with cover > 0.5 are the 18-wide site
    at 213, under the structure PFM alone and under both -- the arg-max window of the golden thresholded scan"""
    from rnascan_amd import fasta, footprint, pack, pssm
    d, sid = hist_dir(tmp_path)
    seq = "".join(ln.strip() for ln in open(HIST_FA).read().splitlines()[1:]).upper().replace("T", "U")
    letters, rows = fasta.read_profile(HIST_PROFILE)
    s_odds = next(iter(pssm.load_odds(SLBP_STRUCT, 0.0, fasta.STRUCT, None).values()))
    q_odds = next(iter(pssm.load_odds(SLBP_SEQ, 0.0, fasta.RNA, None).values()))
    S = np.stack([s_odds[c] for c in letters], axis=1)               # the stored column order of the file
    codes = np.array([pack.RNA_LETTERS.index(c) if c in pack.RNA_LETTERS else 7 for c in seq], dtype=np.uint8)
    assert S.shape[0] == 18 and rows.shape == (len(seq), 7)
    for opts, inputs, R, lo, hi in ((["-q", SLBP_STRUCT], [d], None, 0.9975, 0.9976), (["-p", SLBP_SEQ, "-q", SLBP_STRUCT], [HIST_FA, d],
                                                                                    q_odds.ratio_table(pack.RNA_LETTERS), 0.999998, 0.999999)):
        rc, text = run_command(rules.RulesEngine(), opts + ["-u", "-C", "0", "--pairing", "aligned"] + inputs)
        assert rc == 0
        lines = text.splitlines()
        assert lines[0].split("\t") == footprint.COLUMNS and len(lines) == 2
        row = lines[1].split("\t")
        assert row[1] == sid and row[2:4] == ["213", "230"] and 213 <= int(row[4]) <= 230
        # the covers by the rules, not retyped
        start, cover, occ, _ = rules.footprint(rows, [0], [len(seq)], S, codes, R, rules.POSTERIOR)
        assert list(np.flatnonzero(cover[0] > 0.5) + 1) == list(range(213, 231))
        assert int(np.argmax(start[0])) + 1 == 213 and lo < start[0, 212] < hi
        assert float(row[5]) == cover[0].max() and int(row[4]) == int(np.argmax(cover[0])) + 1 and float(row[6]) == start[0, 212]
    # the structure PFM alone finds the site with a pseudocount too
    rc, text = run_command(rules.RulesEngine(), ["-q", SLBP_STRUCT, "-u", "-C", "0.01", d])
    assert rc == 0 and [ln.split("\t")[2:4] for ln in text.splitlines()[1:]] == [["213", "230"]]
    case = next(c for c in golden["pwm"] if c["name"] == "hist_slbp_pc0_uniform")
    assert case["sequence"] == seq and int(np.argmax(np.asarray(case["scores"]))) + 1 == 213


@pytest.mark.parametrize("weight", ["posterior", "ratio"])
def test_command_directory_store_batches_and_positions(tmp_path, weight):
    from rnascan_amd import expect, footprint, pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.01, "GAUC", None).values()))
    mode = expect.MODES[weight]
    thr = 0.05 if weight == "posterior" else 2.0
    base = ["-u", "-C", "0.01", "--weight", weight, "--min-cover", str(thr)]
    for opts, inputs, qo, ids, mid in ((["-q", stp], [d], None, dir_order(d), "st"), (["-p", seq, "-q", stp], [fa, d], q_odds, order, "seq")):
        for positions in (False, True):
            extra = ["--positions"] if positions else []
            rc, text = run_command(rules.RulesEngine(), opts + base + extra + inputs)
            assert rc == 0
            lines = text.splitlines(True)
            assert lines[0] == "\t".join(footprint.POSITION_COLUMNS if positions else footprint.COLUMNS) + "\n"
            want = []
            for sid in ids:                                          # a directory alone: its own order; with a FASTA: the FASTA's
                want += rule_lines(data, sid, lines[1].split("\t")[0] if len(lines) > 1 else mid, s_odds, qo, mode, thr, positions)[0]
            assert lines[1:] == want and len(want) > 5
            # with a FASTA the store gives the same bytes; alone its order is its own (sorted; the directory's is the file system's)
            stored = text if qo is not None else lines[0] + "".join(
                "".join(rule_lines(data, sid, lines[1].split("\t")[0], s_odds, qo, mode, thr, positions)[0]) for sid in dir_order(st))
            assert sorted(stored.splitlines()) == sorted(text.splitlines())
            for more, inp in ((["--batch-records", "1"], inputs), (["--batch-records", "2"], inputs), (["--batch-records", "1000"], inputs),
                              ([], inputs[:-1] + [st]), (["--batch-records", "2"], inputs[:-1] + [st])):
                e = rules.RulesEngine()
                assert run_command(e, opts + base + extra + more + inp) == (0, stored if inp[-1] == st else text)
                if more == ["--batch-records", "1"]:
                    assert len(e.calls) == 6
    # --profile-dtype float32 rounds the rows first: the rules on float32 rows
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "--profile-dtype", "float32"] + base + [d])
    want = []
    for sid in dir_order(d):
        want += rule_lines(data, sid, text.splitlines()[1].split("\t")[0], s_odds, None, mode, thr, False, dtype=np.float32)[0]
    assert rc == 0 and text.splitlines(True)[1:] == want


def test_command_two_column_orders_in_one_directory(tmp_path):
    """files of two stored column orders: every record gets the value of ITS order (the marginal adds in the stored order)"""
    from rnascan_amd import pssm
    other = "EHTBLRM"
    orders = [FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER]
    fa, mixed, _, data, order = make_inputs(tmp_path, orders=orders, name="mixed")
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.0, "EHTBLRM", None).values()))
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "-u", "--positions", "--min-cover", "0.02", mixed])
    assert rc == 0
    lines = text.splitlines(True)[1:]
    mid = lines[0].split("\t")[0]
    own, plain = [], []
    for sid in dir_order(mixed):
        own += rule_lines(data, sid, mid, s_odds, None, rules.POSTERIOR, 0.02, True, cols=orders[int(sid[1:])])[0]
        plain += rule_lines(data, sid, mid, s_odds, None, rules.POSTERIOR, 0.02, True)[0]
    assert lines == own and lines != plain
    for n in ("1", "2"):
        assert run_command(rules.RulesEngine(), ["-q", stp, "-u", "--positions", "--min-cover", "0.02", "--batch-records", n, mixed])[1] == text


def test_command_all_motifs_row_order_and_the_default_background(tmp_path, capsys):
    from rnascan_amd import background, pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    widths, ids = (6, 4, 6), ["A", "B", "C"]
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", widths, seed=2, ids=ids)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, widths, seed=3, ids=ids)
    for opts, inputs, recs in ((["-q", stp], [d], dir_order(d)), (["-p", seq, "-q", stp], [fa, d], order)):
        argv = opts + ["-u", "-C", "0.01", "--all-motifs", "--positions", "--min-cover", "0.05"]
        rc, text = run_command(rules.RulesEngine(), argv + inputs)
        assert rc == 0
        rows = [ln.split("\t") for ln in text.splitlines()[1:]]
        keys = [(recs.index(r[1]), ids.index(r[0]), int(r[2])) for r in rows]
        assert keys == sorted(keys) and len({k[1] for k in keys}) == 3 and len(rows) > 20   # record, then the file's motif order, then position
        for n in ("1", "4"):
            assert run_command(rules.RulesEngine(), argv + ["--batch-records", n] + inputs)[1] == text
        first = run_command(rules.RulesEngine(), opts + ["-u", "-C", "0.01", "--positions", "--min-cover", "0.05"] + inputs)[1].splitlines()
        assert first[1:] == [ln for ln, k in zip(text.splitlines()[1:], keys) if k[1] == 0]
        assert "have occupancy 0 and no row" in capsys.readouterr().err       # r1 is 3 rows long: no window
    # without -u / -B the structure background is the profiles' own
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "-C", "0.01", "--positions", "--min-cover", "0.05", d])
    bg = background.profile_background(rules.RulesEngine(), d)
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", bg).values()))
    want = []
    for sid in dir_order(d):
        want += rule_lines(data, sid, "A", s_odds, None, rules.POSTERIOR, 0.05, True)[0]
    assert rc == 0 and text.splitlines(True)[1:] == want
    assert text != run_command(rules.RulesEngine(), ["-q", stp, "-u", "-C", "0.01", "--positions", "--min-cover", "0.05", d])[1]


def test_errors_before_a_device_is_opened(tmp_path, capsys):
    """exit 1, a message that names the cause, nothing written; engine None: a device would be opened (and fail here) if the
    check came later"""
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    seq5 = write_pfm(tmp_path / "seq5.pfm", "ACGU", (5,))
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    wide = write_pfm(tmp_path / "wide.pfm", STRUCT, (65,))
    for argv, needles in (([d], ("-q",)),
                          (["-p", seq, fa, d], ("-q", "rnascan_amd.footprint")),                       # -p alone
                          (["-q", stp, fa], ("not an averaged-structure", "rnascan_amd.footprint")),     # a FASTA as the last input
                          (["-p", seq, "-q", stp, d, fa], ("not an averaged-structure",)),
                          (["-p", seq, "-q", stp, d], ("-p with -q needs the sequence FASTA",)),         # -p -q with one input
                          (["-p", seq, "-q", stp, d, st], ("sequence FASTA first",)),
                          (["-q", stp, fa, d], ("-q alone takes one input",)),
                          (["-q", wide, "-u", d], ("-q", "PFMSCAN_MAX_M", "65")),
                          (["-p", seq5, "-q", stp, fa, d], ("share no window",)),
                          (["-q", str(tmp_path / "none.pfm"), d], ("none.pfm",))):
        rc, text = run_command(None, argv)
        err = capsys.readouterr().err
        assert rc == 1 and text == "", argv
        for needle in needles:
            assert needle in err, (argv, err)
    with pytest.raises(SystemExit):
        run_command(None, ["-q", stp, "--weight", "ratio", d])
    assert "--min-cover" in capsys.readouterr().err
    # `footprint` itself keeps refusing the directory, and names this command
    from rnascan_amd import footprint
    out = io.StringIO()
    assert footprint.main(["-q", stp, "-u", d], engine=None, out=out) == 1 and out.getvalue() == ""
    assert "rnascan_amd.footprint_profile" in capsys.readouterr().err


def test_input_errors_name_the_record(tmp_path, capsys):
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,))
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    argv = ["-p", seq, "-q", stp, "-u"]
    lines = open(fa).read().splitlines()
    (tmp_path / "long.fa").write_text("\n".join([lines[0], lines[1] + "A"] + lines[2:]) + "\n")      # a length mismatch
    rc, text = run_command(rules.RulesEngine(), argv + [str(tmp_path / "long.fa"), d])
    err = capsys.readouterr().err
    assert rc == 1 and text == "" and lines[0][1:].split()[0] in err and "letters long but its averaged-structure profile has" in err
    (tmp_path / "dup.fa").write_text("\n".join(lines + lines[:2]) + "\n")                           # a duplicate id
    rc, text = run_command(rules.RulesEngine(), argv + [str(tmp_path / "dup.fa"), d])
    err = capsys.readouterr().err
    assert rc == 1 and text == "" and "more than once" in err and lines[0][1:].split()[0] in err
    (tmp_path / "extra.fa").write_text("\n".join(lines + [">nowhere", "ACGUACGUACGU"]) + "\n")       # a record without a profile
    rc, text = run_command(rules.RulesEngine(), argv + [str(tmp_path / "extra.fa"), d])
    err = capsys.readouterr().err
    assert rc == 1 and text == "" and "nowhere" in err


def test_nan_zero_and_negative_occupancies(tmp_path, capsys):
    from rnascan_amd import pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (5,), seed=3)
    # a background of 0 for a letter the motif has: a ratio is +inf, times a zero cell NaN -- exit 1, motif and record named, nothing written
    (tmp_path / "bgs.txt").write_text(repr(dict(zip(STRUCT, (0.0, 0.3, 0.2, 0.2, 0.1, 0.1, 0.1)))))
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "-C", "0.01", "-B", str(tmp_path / "bgs.txt"), d])
    err = capsys.readouterr().err
    assert rc == 1 and text == "" and "Motif st" in err and "record r" in err and ("infinite" in err or "not a number" in err)
    # occupancy 0 (r1 has no window): no row, counted on stderr
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "-u", "-C", "0.01", d])
    err = capsys.readouterr().err
    assert rc == 0 and "1 record x motif pairs have occupancy 0 and no row" in err and "\tr1\t" not in text
    # a record of negative cells under -u: a negative occupancy, and the rows the rules give
    neg = tmp_path / "neg"
    neg.mkdir()
    for sid in ("r0", "r3"):
        write_profile(neg, sid, data[sid][1] * (-1 if sid == "r3" else 1))
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", None).values()))
    flipped = dict(data, r3=(data["r3"][0], -data["r3"][1]))
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "-u", "-C", "0.01", "--positions", "--min-cover", "0.05", str(neg)])
    assert rc == 0
    want, occs = [], {}
    for sid in dir_order(str(neg)):
        got, occs[sid] = rule_lines(flipped, sid, "st", s_odds, None, rules.POSTERIOR, 0.05, True)
        want += got
    assert occs["r0"] > 0 > occs["r3"] and text.splitlines(True)[1:] == want and any("\tr3\t" in ln for ln in want)
