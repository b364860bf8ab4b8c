"""The multi-site model on averaged-structure profiles without a device: the rules (tests/multisite_profile_rules.py) against
an enumeration of every configuration in exact arithmetic and against the letter rules they must reduce to, the reference's
example record, the bindings, and the host logic of `python -m rnascan_amd.multisite_profile` with the rules in the device's
place."""
import io
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

import multisite_profile_rules as rules
import multisite_rules as mrules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import pair_rules
from conftest import DATA_DIR, REPO
from test_occupancy_profile_cpu import FILE_ORDER, STRUCT, make_inputs, write_pfm, write_profile

HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
HIST_PROFILE = os.path.join(DATA_DIR, "HIST2H3C_3p_end_structure.txt")
SLBP_SEQ = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
SLBP_STRUCT = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")
NAMES = ("pfmscan_multisite_profile_dev", "pfmscan_multisite_profile_staged", "pfmscan_multisite_profile_events_dev",
         "pfmscan_multisite_profile_events_staged")


# ---- bindings ----------------------------------------------------------------------------------------------------------
def test_the_header_and_the_bindings_export_the_four_entry_points():
    from rnascan_amd import _lib, build, scanner
    build.build_lib()
    L = _lib.load()
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == L.pfmscan_abi_version() == 27
    for name in NAMES:
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name) is not None
        assert callable(getattr(_lib.Context, name[len("pfmscan_"):]))
    assert "pfmscan_multisite.hip" in build.SOURCES
    assert callable(scanner.HipEngine.multisite_profile) and callable(scanner.HipEngine.multisite_profile_events)


# ---- the rules against every configuration, exactly --------------------------------------------------------------------
def exact_terms(profile, L, S, codes, R):
    """the terms of a record's windows as Fractions of the widened row cells and the table cells: no rounding anywhere"""
    m = S.shape[0]
    out = []
    for s in range(max(L - m + 1, 0)):
        if R is not None and any((int(codes[s + k]) & 7) >= 4 for k in range(m)):
            out.append(Fraction(0))
            continue
        t = Fraction(1)
        for k in range(m):
            if R is not None:
                t *= Fraction(float(R[k][int(codes[s + k]) & 7]))
            t *= sum(Fraction(float(profile[s + k][c])) * Fraction(float(S[k][c])) for c in range(7))
        out.append(t)
    return out


def configurations(n_win, m, s=0):
    """every set of non-overlapping windows of width m among n_win, as tuples of their starts"""
    if s >= n_win:
        yield ()
        return
    for rest in configurations(n_win, m, s + 1):
        yield rest
    for rest in configurations(n_win, m, s + m):
        yield (s,) + rest


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_configuration_in_exact_arithmetic(joint, dtype):
    """Z and start against the sum over every set of non-overlapping windows in Fractions, on non-negative rows.

    The bounds: multisite_rules.z_bound(L) = gamma(2 L) and start_bound(L) = gamma(4 L + 4) hold against the exact model over
    the COMPUTED activities.  A computed activity is the exact one times at most 14 m factors (1 + d), |d| <= U: a marginal puts
    7 roundings on every summand (all of one sign), the chain multiplies m marginals and in joint mode m letter ratios with
    one rounding each, the product with lam is one more: 8 m structure only, 9 m joint, <= 14 m.  A configuration is a product
    of at most floor(L / m) activities, so its weight carries at most A = 14 m floor(L / m) more factors; every weight is
    non-negative, so the sums carry them too: Z is within gamma(2 L + A) of the exact one, and start -- a ratio of two such
    sums -- within gamma(4 L + 4 + 2 A)."""
    rng = np.random.default_rng(40 + joint)
    n_cases = 0
    for m in (1, 2, 3):
        for L in (0, m - 1, m, m + 1, 2 * m, 7, 10):
            L = max(L, 0)
            codes, profile, off, lens = prules.stream(rng, [L], dtype)
            if joint and L > 2:
                codes[int(rng.integers(0, L))] = 5                        # a foreign code: its windows have no term
            S = prules.struct_table(rng, m)
            R = orules.table(rng, m, 4) if joint else None
            lam = np.array([float(rng.uniform(0.05, 2.0))])
            start, cover, z, ns, win = rules.multisite(profile, off, lens, S, codes, R, lam)
            t = exact_terms(profile, L, S, codes, R)
            a = [x * Fraction(float(lam[0])) for x in t]
            n_win = len(t)
            assert win[0] == sum(1 for s in range(n_win) if R is None or all((int(codes[s + k]) & 7) < 4 for k in range(m)))
            Z = Fraction(0)
            through = [Fraction(0)] * n_win
            for conf in configurations(n_win, m):
                w = Fraction(1)
                for s in conf:
                    w *= a[s]
                Z += w
                for s in conf:
                    through[s] += w
            A = 14 * m * (L // m)
            assert rules.z_bound(L) == mrules.gamma(2 * L) and rules.start_bound(L) == mrules.gamma(4 * L + 4)   # the counts that A is added to
            assert abs(Fraction(float(z[0, 0])) - Z) <= Fraction(mrules.gamma(2 * L + A)) * Z
            for s in range(n_win):
                want = through[s] / Z
                assert abs(Fraction(float(start[0, s])) - want) <= Fraction(mrules.gamma(4 * L + 4 + 2 * A)) * want
            assert (start[0, n_win:L] == 0).all() and not np.signbit(start[0, :L]).any()
            assert cover[0, :L].max(initial=0.0) <= rules.cover_bound(L, m)
            n_cases += 1
    assert n_cases == 21


@pytest.mark.parametrize("m", [1, 5, 12])
def test_one_hot_rows_reduce_to_the_letter_rules(m):
    """rows with a single 1 and finite tables: the marginal is the table cell exactly, so structure only is the model of the
    structure table over the letter codes and joint is the pair chain over (codes, letter codes), bit for bit"""
    rng = np.random.default_rng(300 + m)
    codes, letters, off, lens = pair_rules.streams(rng, [0, m - 1, m, 2 * m + 3, 150, 400], foreign_seq=0.01, foreign_struct=0.0)
    S = prules.struct_table(rng, m)
    S8 = np.full((m, 8), np.nan)
    S8[:, :7] = S
    R = orules.table(rng, m, 4)
    lam = rng.uniform(0.001, 0.1, size=len(off))
    for dtype in (np.float32, np.float64):
        profile = prules.one_hot(letters, dtype)
        got = rules.multisite(profile, off, lens, S, None, None, lam)
        want = mrules.multisite(None, letters, off, lens, None, S8, lam)
        assert all(rules.same_bits(g, w) for g, w in zip(got[:4], want[:4])) and np.array_equal(got[4], want[4])
        got = rules.multisite(profile, off, lens, S, codes, R, lam)
        want = mrules.multisite(codes, letters, off, lens, R, S8, lam)
        assert all(rules.same_bits(g, w) for g, w in zip(got[:4], want[:4])) and np.array_equal(got[4], want[4])
        assert np.isfinite(got[2]).all() and (got[2] >= 1.0).all()


def negative_rows(rows):
    """one negative cell, large enough that the windows over it outweigh everything else: Z < 0"""
    rows = np.array(rows, dtype=np.float64)
    rows[len(rows) // 2] = -50.0
    return rows


def test_the_rule_returns_a_z_that_is_not_positive_or_not_finite():
    rng = np.random.default_rng(5)
    m = 5
    codes, profile, off, lens = prules.stream(rng, [60], np.float64)
    S = prules.struct_table(rng, m)
    profile[:60] = negative_rows(profile[:60])
    start, cover, z, ns, win = rules.multisite(profile, off, lens, S, None, None, np.array([1.0]))
    assert z[0, 0] <= 0.0 and np.isfinite(z[0, 0]) and win[0] == 56                       # every window has a term, negative ones too
    profile[:60] = np.abs(profile[:60])
    start, cover, z, ns, win = rules.multisite(profile, off, lens, S, None, None, np.array([1e300]))
    assert not np.isfinite(z[0, 0])


# ---- the command with the rules in the device's place ------------------------------------------------------------------
def run_command(engine, argv):
    from rnascan_amd import multisite_profile
    out = io.StringIO()
    rc = multisite_profile.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def rule_lines(data, sid, mid, struct_odds, seq_odds, thr, positions, prior=1.0, lam=None, cols=FILE_ORDER, dtype=np.float64):
    """the lines of one record under one motif as the rules, footprint.format_rows and multisite.record_rows give them, the
    rows stored in column order ``cols`` -> (lines, --records lines)"""
    from rnascan_amd import footprint, multisite
    seq, rows = data[sid]
    profile = np.ascontiguousarray(rows[:, [STRUCT.index(c) for c in cols]]).astype(dtype)
    S = np.stack([struct_odds[c] for c in cols], axis=1)
    codes = np.array(["ACGU".index(c) if c in "ACGU" else 7 for c in seq], dtype=np.uint8)
    R = None if seq_odds is None else seq_odds.ratio_table("ACGU")
    la = multisite.lam_of([len(seq)], S.shape[0], prior, lam)
    start, cover, z, ns, win = rules.multisite(profile, [0], [len(seq)], S, codes, R, la)
    key, c, w = rules.events(start, cover, [0], [len(seq)], thr)
    return (footprint.format_rows(mid, sid, key, c, w, S.shape[0], positions),
            multisite.record_rows([mid], [sid], win[:, None], z, ns))


def dir_order(d):
    from rnascan_amd import sites
    return list(sites._Profiles(d, np.float64).ids)


def test_command_directory_store_batches_positions_and_records(tmp_path):
    from rnascan_amd import footprint, multisite, pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", None).values()))
    q_odds = next(iter(pssm.load_odds(seq, 0.01, "GAUC", None).values()))
    thr = 0.05
    base = ["-u", "-C", "0.01", "--min-cover", str(thr)]
    for opts, inputs, qo, ids in ((["-q", stp], [d], None, dir_order(d)), (["-p", seq, "-q", stp], [fa, d], q_odds, order)):
        for positions in (False, True):
            recs_path = str(tmp_path / "recs.tsv")
            extra = (["--positions"] if positions else []) + ["--records", recs_path]
            rc, text = run_command(rules.RulesEngine(), opts + base + extra + inputs)
            assert rc == 0
            lines = text.splitlines(True)
            assert lines[0] == "\t".join(footprint.POSITION_COLUMNS if positions else footprint.COLUMNS) + "\n"
            mid = lines[1].split("\t")[0]
            want, want_recs = [], []
            for sid in ids:                                          # a directory alone: its own order; with a FASTA: the FASTA's
                a, b = rule_lines(data, sid, mid, s_odds, qo, thr, positions)
                want += a
                want_recs += b
            rec_text = open(recs_path).read()
            assert lines[1:] == want and len(want) > 5
            assert rec_text.splitlines(True) == ["\t".join(multisite.RECORD_COLUMNS) + "\n"] + want_recs and len(want_recs) == 6
            # with a FASTA the store gives the same bytes; alone its order is its own: the same lines, record by record
            for more, inp in ((["--batch-records", "1"], inputs), (["--batch-records", "2"], inputs), (["--batch-records", "1000"], inputs),
                              ([], inputs[:-1] + [st]), (["--batch-records", "2"], inputs[:-1] + [st])):
                e = rules.RulesEngine()
                os.remove(recs_path)
                rc, got = run_command(e, opts + base + extra + more + inp)
                assert rc == 0
                if inp[-1] == st and qo is None:
                    assert sorted(got.splitlines()) == sorted(text.splitlines()) and sorted(open(recs_path).read().splitlines()) == sorted(rec_text.splitlines())
                    assert got == run_command(rules.RulesEngine(), opts + base + extra + ["--batch-records", "1"] + inp)[1]
                else:
                    assert got == text and open(recs_path).read() == rec_text
                if more == ["--batch-records", "1"]:
                    assert len(e.calls) == 6
    # --profile-dtype float32 rounds the rows first: the rules on float32 rows
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "--profile-dtype", "float32"] + base + [d])
    want = []
    for sid in dir_order(d):
        want += rule_lines(data, sid, text.splitlines()[1].split("\t")[0], s_odds, None, thr, False, dtype=np.float32)[0]
    assert rc == 0 and text.splitlines(True)[1:] == want


def test_command_prior_sites_against_lambda(tmp_path):
    from rnascan_amd import pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", None).values()))
    texts = {}
    for flags, kw in ((["--prior-sites", "0.25"], dict(prior=0.25)), (["--lambda", "0.02"], dict(lam=0.02)), ([], dict(prior=1.0))):
        rc, text = run_command(rules.RulesEngine(), ["-q", stp, "-u", "-C", "0.01", "--positions", "--min-cover", "0.05"] + flags + [d])
        want = []
        for sid in dir_order(d):
            want += rule_lines(data, sid, "st", s_odds, None, 0.05, True, **kw)[0]
        assert rc == 0 and text.splitlines(True)[1:] == want and len(want) > 0
        texts[tuple(flags)] = text
    assert len(set(texts.values())) == 3
    with pytest.raises(SystemExit):
        run_command(rules.RulesEngine(), ["-q", stp, "--prior-sites", "1", "--lambda", "1", d])


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
        own += rule_lines(data, sid, mid, s_odds, None, 0.02, True, cols=orders[int(sid[1:])])[0]
        plain += rule_lines(data, sid, mid, s_odds, None, 0.02, True)[0]
    assert lines == own and lines != plain
    for n in ("1", "2"):
        assert run_command(rules.RulesEngine(), ["-q", stp, "-u", "--positions", "--min-cover", "0.02", "--batch-records", n, mixed])[1] == text


def test_command_all_motifs_row_order_and_the_default_background(tmp_path):
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
    # without -u / -B the structure background is the profiles' own
    rc, text = run_command(rules.RulesEngine(), ["-q", stp, "-C", "0.01", "--positions", "--min-cover", "0.05", d])
    bg = background.profile_background(rules.RulesEngine(), d)
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", bg).values()))
    want = []
    for sid in dir_order(d):
        want += rule_lines(data, sid, "A", s_odds, None, 0.05, True)[0]
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
                          (["-p", seq, fa, d], ("-q", "rnascan_amd.multisite")),                        # -p alone
                          (["-q", stp, fa], ("not an averaged-structure", "rnascan_amd.multisite")),      # a FASTA as the last input
                          (["-p", seq, "-q", stp, d, fa], ("not an averaged-structure",)),
                          (["-p", seq, "-q", stp, d], ("-p with -q needs the sequence FASTA",)),          # -p -q with one input
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
    for bad in (["--min-cover", "nan"], ["--lambda", "-1"], ["--prior-sites", "inf"]):
        with pytest.raises(SystemExit):
            run_command(None, ["-q", stp] + bad + [d])
        capsys.readouterr()


def test_multisite_on_letters_keeps_refusing_a_directory(tmp_path, capsys):
    from rnascan_amd import multisite
    fa, d, st, data, order = make_inputs(tmp_path)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    for path in (d, st):
        out = io.StringIO()
        assert multisite.main(["-q", stp, "-u", path], engine=None, out=out) == 1 and out.getvalue() == ""
        assert capsys.readouterr().err.strip() == (
            "%s is an averaged-structure directory or packed store: the multi-site model takes FASTA files of letters "
            "(averaged-structure profiles are not supported by this command)" % path)


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


def test_a_z_that_is_not_positive_or_not_finite_exits_1_and_writes_nothing(tmp_path, capsys):
    from rnascan_amd import pssm
    fa, d, st, data, order = make_inputs(tmp_path)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (5,), seed=3)
    s_odds = next(iter(pssm.load_odds(stp, 0.01, "EHTBLRM", None).values()))
    neg = tmp_path / "neg"
    neg.mkdir()
    changed = dict(data, r3=(data["r3"][0], negative_rows(data["r3"][1])))
    for sid in ("r0", "r3"):
        write_profile(neg, sid, changed[sid][1])
    recs_path = str(tmp_path / "recs.tsv")
    argv = ["-q", stp, "-u", "-C", "0.01", "--records", recs_path]
    # the rule returns the Z the command refuses
    S = np.stack([s_odds[c] for c in FILE_ORDER], axis=1)
    rows = np.ascontiguousarray(changed["r3"][1][:, [STRUCT.index(c) for c in FILE_ORDER]])
    z = rules.multisite(rows, [0], [len(rows)], S, None, None, np.array([0.5]))[2]
    assert z[0, 0] <= 0.0 and np.isfinite(z[0, 0])
    rc, text = run_command(rules.RulesEngine(), argv + ["--lambda", "0.5", str(neg)])
    err = capsys.readouterr().err
    assert rc == 1 and text == "" and not os.path.exists(recs_path)
    assert "Motif st" in err and "record r3" in err and "zero or negative" in err and "negative profile cells" in err
    # an infinite Z: the record is named too, by multisite's own message
    z = rules.multisite(np.ascontiguousarray(data["r0"][1][:, [STRUCT.index(c) for c in FILE_ORDER]]), [0], [len(data["r0"][1])], S, None, None,
                        np.array([1e300]))[2]
    assert not np.isfinite(z[0, 0])
    rc, text = run_command(rules.RulesEngine(), argv + ["--lambda", "1e300", d])
    err = capsys.readouterr().err
    assert rc == 1 and text == "" and not os.path.exists(recs_path)
    assert "Motif st" in err and "record r" in err and "infinite or not a number" in err
    # the same records with a lam that leaves Z positive: rows
    rc, text = run_command(rules.RulesEngine(), argv + ["--lambda", "1e-9", str(neg)])
    assert rc == 0 and os.path.exists(recs_path) and len(open(recs_path).read().splitlines()) == 3


# ---- the reference's example ------------------------------------------------------------------------------------------
def hist_dir(tmp_path):
    d = tmp_path / "hist"
    d.mkdir()
    sid = open(HIST_FA).readline()[1:].split()[0]
    shutil.copyfile(HIST_PROFILE, d / ("structure.%s.txt" % sid))
    return str(d), sid


def test_the_example_record(tmp_path):
    """the reference's example record, its averaged-structure profile and the two SLBP PFMs, -u -C 0, aligned pairing: the joint
    model at --prior-sites 0.01 prints the one region 213 230, the known site; the structure PFM alone is promiscuous under
    this model (expected odds on near-one-hot rows are large with pseudocount 0).  Every value by the rules, not retyped; the
    ranges are DESIGN.md 5n's table"""
    from rnascan_amd import fasta, footprint, multisite, pack, pssm
    d, sid = hist_dir(tmp_path)
    seq = "".join(ln.strip() for ln in open(HIST_FA).read().splitlines()[1:]).upper().replace("T", "U")
    letters, rows = fasta.read_profile(HIST_PROFILE)
    s_odds = next(iter(pssm.load_odds(SLBP_STRUCT, 0.0, fasta.STRUCT, None).values()))
    q_odds = next(iter(pssm.load_odds(SLBP_SEQ, 0.0, fasta.RNA, None).values()))
    S = np.stack([s_odds[c] for c in letters], axis=1)               # the stored column order of the file
    R = q_odds.ratio_table(pack.RNA_LETTERS)
    codes = np.array([pack.RNA_LETTERS.index(c) if c in pack.RNA_LETTERS else 7 for c in seq], dtype=np.uint8)
    L = len(seq)
    assert S.shape[0] == 18 and rows.shape == (L, 7)
    site = list(range(213, 231))

    def model(Rq, G):
        start, cover, z, ns, _ = rules.multisite(rows, [0], [L], S, codes, Rq, multisite.lam_of([L], 18, G, None))
        return start[0], cover[0], float(z[0, 0]), float(ns[0, 0]), list(np.flatnonzero(cover[0] > 0.5) + 1)

    # structure only
    start, cover, z, ns, pos = model(None, 1.0)
    assert 2.4e33 < z < 2.6e33 and 7.71 < ns < 7.73 and len(pos) == 144 and (pos[0], pos[-1]) == (11, 230) and 0.99755 < start[212] < 0.99756
    start, cover, z, ns, pos = model(None, 0.001)
    assert 3.2e14 < z < 3.4e14 and 4.76 < ns < 4.78 and pos != site and 0.99755 < start[212] < 0.99756
    # joint
    start, cover, z, ns, pos = model(R, 1.0)
    assert 2.5e18 < z < 2.7e18 and 4.53 < ns < 4.55 and len(pos) == 88 and 0.999998 < start[212] < 0.999999
    start, cover, z, ns, pos = model(R, 0.001)
    assert 1.04 < ns < 1.05 and pos == site and 0.999998 < start[212] < 0.999999
    start, cover, z, ns, pos = model(R, 0.01)
    assert 5.75e12 < z < 5.77e12 and 1.40 < ns < 1.41 and pos == site and 0.999998 < start[212] < 0.999999
    # the command
    recs_path = str(tmp_path / "recs.tsv")
    rc, text = run_command(rules.RulesEngine(), ["-p", SLBP_SEQ, "-q", SLBP_STRUCT, "-u", "-C", "0", "--pairing", "aligned", "--prior-sites", "0.01",
                                                  "--records", recs_path, HIST_FA, d])
    assert rc == 0
    lines = text.splitlines()
    assert lines[0].split("\t") == footprint.COLUMNS and len(lines) == 2
    row = lines[1].split("\t")
    assert row[1] == sid and row[2:4] == ["213", "230"]
    assert float(row[5]) == cover[212:230].max() and int(row[4]) == 213 + int(np.argmax(cover[212:230])) and float(row[6]) == start[212]
    rec = open(recs_path).read().splitlines()[1].split("\t")
    assert rec[1] == sid and int(rec[2]) == L - 17 and float(rec[3]) == z and float(rec[5]) == (z - 1.0) / z and float(rec[6]) == ns
    # the structure PFM alone at the default prior: several regions
    rc, text = run_command(rules.RulesEngine(), ["-q", SLBP_STRUCT, "-u", "-C", "0", d])
    assert rc == 0 and len(text.splitlines()) > 3 and text.splitlines()[-1].split("\t")[3] == "230"
