"""The multi-site model on the CPU: the rules (tests/multisite_rules.py) against a brute-force enumeration of every set of
non-overlapping sites in exact arithmetic, their closed forms and identities within bounds derived in the rules file, the
reference's example record, and the host logic of `python -m rnascan_amd.multisite` with the rules in the device's place."""
import io
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import footprint_rules as frules
import multisite_rules as rules
from conftest import DATA_DIR, REPO
from test_footprint_cpu import RNA, STRUCT, planted
from test_occupancy_cpu import write_pfm
from test_pair_cpu import SEQS, write_inputs

HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
SLBP_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")


def brute(a, L, m):
    """every set of non-overlapping windows, in Fractions of the activities as doubles -> (Z, [posterior of a site at s])"""
    n_win = max(L - m + 1, 0)
    a = [Fraction(float(x)) for x in a]
    Z, at = Fraction(0), [Fraction(0)] * n_win
    for k in range(0, n_win + 1):
        for sites in itertools.combinations(range(n_win), k):
            if all(sites[i + 1] - sites[i] >= m for i in range(k - 1)):
                w = Fraction(1)
                for s in sites:
                    w *= a[s]
                Z += w
                for s in sites:
                    at[s] += w
    return Z, [x / Z for x in at]


def record(rng, L, m, foreign=0.1):
    codes, off, lens = rules.stream(rng, [L], 4, foreign=foreign)
    R = rules.table(rng, m, 4)
    t, has = frules.record_terms(codes, None, 0, L, R, None)
    return codes, R, t, has


@pytest.mark.parametrize("m", [1, 2, 3])
def test_brute_force_over_every_configuration(m):
    rng = np.random.default_rng(100 + m)
    worst = 0.0
    for L in range(0, 11):
        for _ in range(6):
            codes, R, t, has = record(rng, L, m)
            lam = float(rng.uniform(0.0, 3.0))
            a = rules.activities(t, lam)
            start, cover, Z, ns = rules.model_of_terms(t, lam, L, m)
            Zx, px = brute(a, L, m)
            assert abs(Fraction(Z) - Zx) <= Fraction(rules.z_bound(L)) * Zx
            worst = max(worst, float(abs(Fraction(Z) - Zx) / Zx) / rules.U)
            for s, p in enumerate(px):
                assert abs(Fraction(float(start[s])) - p) <= Fraction(rules.start_bound(L)) * p
                if p:
                    worst = max(worst, float(abs(Fraction(float(start[s])) - p) / p) / rules.U)
            assert (start[len(px):] == 0).all() and not np.signbit(start).any()
            F, B = rules.forward(a, L, m), rules.backward(a, L, m)
            assert abs(Fraction(F[L]) - Fraction(B[0])) <= 2 * Fraction(rules.z_bound(L)) * Zx
            assert all(F[i + 1] >= F[i] for i in range(L)) and not any(np.signbit(x) for x in F + B)
            if L:
                assert cover.max() <= rules.cover_bound(L, m)
            exact = rules.exact_sum(start)
            assert abs(Fraction(ns) - exact) <= Fraction(rules.nsites_bound(len(px))) * exact
            # the occupancy is the first-order term; independent sites are the upper bound
            first = 1 + sum(Fraction(x) for x in a)
            prod = Fraction(1)
            for x in a:
                prod *= 1 + Fraction(x)
            assert first * (1 - Fraction(rules.z_bound(L))) <= Fraction(Z) <= prod * (1 + Fraction(rules.z_bound(L)))
    assert worst < 4 * 10 + 4                                       # far inside gamma(4 L + 4) at L = 10; said so that a regression shows


def test_closed_forms():
    rng = np.random.default_rng(7)
    # m = 1: windows do not compete: Z = prod (1 + a_s) and start[s] = a_s / (1 + a_s), exactly in Fractions
    for L in (1, 5, 9):
        codes, R, t, has = record(rng, L, 1)
        lam = 0.7
        a = rules.activities(t, lam)
        Zx, px = brute(a, L, 1)
        prod = Fraction(1)
        for x in a:
            prod *= 1 + Fraction(x)
        assert Zx == prod and px == [Fraction(x) / (1 + Fraction(x)) for x in a]
    # L = m: one window
    for m in (1, 4, 9):
        codes, R, t, has = record(rng, m, m, foreign=0.0)
        lam = 0.3
        start, cover, Z, ns = rules.model_of_terms(t, lam, m, m)
        a0 = float(t[0]) * lam
        assert Z == 1.0 + a0 * 1.0 and start[0] == ((1.0 * a0) * 1.0) * (1.0 / Z) and ns == start[0]
        assert (cover == start[0]).all()
    # lam = +0.0: the empty configuration alone; L < m: no window
    codes, R, t, has = record(rng, 40, 5)
    start, cover, Z, ns = rules.model_of_terms(t, 0.0, 40, 5)
    assert Z == 1.0 and ns == 0.0 and (start == 0).all() and (cover == 0).all() and not np.signbit(start).any() and not np.signbit(cover).any()
    start, cover, Z, ns = rules.model_of_terms(np.zeros(0), 0.5, 3, 5)
    assert Z == 1.0 and ns == 0.0 and start.shape == (3,) and (cover == 0).all()
    start, cover, Z, ns = rules.model_of_terms(np.zeros(0), 0.5, 0, 5)
    assert Z == 1.0 and start.shape == (0,)


def test_the_order_of_the_additions_is_part_of_the_rule():
    """activities whose posteriors add up differently in another order: nsites runs from the last window down, cover from the
    lowest start up"""
    m = 1
    big, small = 1.0, 2.0 ** -54
    # m = 1: start[s] = a_s / (1 + a_s) up to rounding; the small ones are lost against the big one unless they are added first
    t = np.array([big, small, small, small])
    start, cover, Z, ns = rules.model_of_terms(t, 1.0, 4, m)
    down = ((0.0 + start[3]) + start[2] + start[1]) + start[0]
    up = ((0.0 + start[0]) + start[1] + start[2]) + start[3]
    assert ns == down and down != up
    # cover: maps_of_weights unchanged, ascending
    w = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 1.0])
    _, c = frules.maps_of_weights(w, 6, 3)
    assert c[2] == 1.0 and c[3] == 1.0 + 2.0 ** -52
    # a foreign code: the window has no term, its activity is +0.0 and it never starts a site
    rng = np.random.default_rng(3)
    codes, off, lens = rules.stream(rng, [30], 4)
    codes[12] = 5
    R = rules.table(rng, 4, 4)
    start, cover, z, ns, win = rules.multisite(codes, None, off, lens, R, None, np.array([0.5]))
    assert (start[0, 9:13] == 0).all() and win[0] == 27 - 4 and start[0, 8] > 0 and start[0, 13] > 0


def test_the_header_and_the_bindings_export_the_multisite_entry_points():
    from rnascan_amd import _lib, build, scanner
    text = open(os.path.join(REPO, "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 27
    assert int(re.search(r"#define\s+PFMSCAN_MULTISITE_SLOTS\s+(\d+)", text).group(1)) == _lib.MULTISITE_SLOTS
    assert int(re.search(r"#define\s+PFMSCAN_MULTISITE_CHUNK\s+(\d+)", text).group(1)) == _lib.MULTISITE_CHUNK
    for name in ("pfmscan_multisite_dev", "pfmscan_multisite_staged", "pfmscan_multisite_events_dev", "pfmscan_multisite_events_staged"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text)
        assert hasattr(_lib.Context, name[len("pfmscan_"):])
    assert "pfmscan_multisite.hip" in build.SOURCES
    assert hasattr(scanner.HipEngine, "multisite") and hasattr(scanner.HipEngine, "multisite_events")


# ---- the command with the rules in the device's place ------------------------------------------------------------------
def run_command(engine, argv):
    from rnascan_amd import multisite
    out = io.StringIO()
    rc = multisite.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def hist_by_the_rules(prior):
    from rnascan_amd import fasta, pack, pssm
    odds = pssm.load_odds(SLBP_PFM, 0.0, fasta.RNA, None)
    mid = next(iter(odds))
    R = odds[mid].ratio_table(pack.RNA_LETTERS)
    seq = "".join(ln.strip() for ln in open(HIST_FA).read().splitlines()[1:]).upper().replace("T", "U")
    codes = np.array([pack.RNA_LETTERS.index(c) if c in pack.RNA_LETTERS else 7 for c in seq] + [7], dtype=np.uint8)
    L, m = len(seq), R.shape[0]
    lam = np.array([prior / max(L - m + 1, 1)])
    return mid, L, m, lam, rules.multisite(codes, None, [0], [L], R, None, lam)


def test_the_known_slbp_site_and_the_empty_configuration(tmp_path):
    """the reference's example record under the SLBP motif.  At one site a priori the site at 213 is found as footprint finds
    it; at a hundredth of a site the record is more likely unbound than bound and NO region is reported -- the empty
    configuration, which one site per record cannot express"""
    from rnascan_amd import multisite
    rec = str(tmp_path / "records.tsv")
    base = ["-p", SLBP_PFM, "-u", "-C", "0", HIST_FA, "--records", rec]
    mid, L, m, lam, (start, cover, z, ns, win) = hist_by_the_rules(1.0)
    assert m == 18 and L - m + 1 == 219 and lam[0] == 1.0 / 219
    rc, text = run_command(rules.RulesEngine(), base)
    lines = text.splitlines()
    assert rc == 0 and lines[0].split("\t") == multisite.COLUMNS and len(lines) == 2
    row = lines[1].split("\t")
    assert row[:4] == [mid, row[1], "213", "230"]
    assert list(np.flatnonzero(cover[0] > 0.5) + 1) == list(range(213, 231))
    assert 93.7 < z[0, 0] < 93.9 and 0.987 < start[0, 212] < 0.9876 and 1.02 < ns[0, 0] < 1.025
    assert float(row[5]) == cover[0].max() and int(row[4]) == int(np.argmax(cover[0])) + 1 and float(row[6]) == start[0, 212]
    rlines = open(rec).read().splitlines()
    assert rlines[0].split("\t") == multisite.RECORD_COLUMNS and len(rlines) == 2
    r = rlines[1].split("\t")
    assert r[0] == mid and int(r[2]) == win[0] == 219 and float(r[3]) == z[0, 0] and r[3] == repr(float(z[0, 0]))
    assert float(r[5]) == (z[0, 0] - 1.0) / z[0, 0] and 0.989 < float(r[5]) < 0.9895 and float(r[6]) == ns[0, 0]
    assert r[4] == repr(round(float(np.log2(z[0, 0])), 3))
    # a tenth of a site a priori: the same region
    rc, text = run_command(rules.RulesEngine(), base + ["--prior-sites", "0.1"])
    assert rc == 0 and [ln.split("\t")[2:4] for ln in text.splitlines()[1:]] == [["213", "230"]]
    # a hundredth: no region
    _, _, _, _, (start, cover, z, ns, win) = hist_by_the_rules(0.01)
    rc, text = run_command(rules.RulesEngine(), base + ["--prior-sites", "0.01"])
    assert rc == 0 and text.splitlines()[1:] == []
    assert 0.47 < cover[0].max() < 0.476 and 0.47 < (z[0, 0] - 1.0) / z[0, 0] < 0.476
    assert float(open(rec).read().splitlines()[1].split("\t")[5]) == (z[0, 0] - 1.0) / z[0, 0]
    # --lambda: the same activity said directly
    rc, text2 = run_command(rules.RulesEngine(), ["-p", SLBP_PFM, "-u", "-C", "0", HIST_FA, "--lambda", repr(1.0 / 219)])
    assert rc == 0 and text2 == run_command(rules.RulesEngine(), base)[1]


def test_command_regions_positions_records_and_batching(tmp_path):
    from rnascan_amd import multisite
    fa, recs, site = planted(tmp_path)
    rec = str(tmp_path / "rec.tsv")
    base = ["-p", SLBP_PFM, "-u", "-C", "0.01"]
    rc, text = run_command(rules.RulesEngine(), base + [fa, "--records", rec])
    assert rc == 0
    rtext = open(rec).read()
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    by_rec = {}
    for r in rows:
        by_rec.setdefault(r[1], []).append(r)
    m = len(site)
    # any number of sites: both planted sites of `twice` are regions at the default threshold, `none` has no region at all
    assert set(by_rec) == {"first", "last", "twice", "lower"} and len(by_rec["twice"]) == 2
    assert [int(r[2]) for r in by_rec["twice"]] == [31, 31 + m + 40]
    assert by_rec["first"][0][2] == "1" and by_rec["last"][-1][3] == str(len(recs[1][1]))
    rrows = [ln.split("\t") for ln in rtext.splitlines()[1:]]
    assert [r[1] for r in rrows] == [i for i, _ in recs]                    # every record, in order
    got = dict((r[1], r) for r in rrows)
    assert got["short"][2:] == ["0", "1.0", "0.0", "0.0", "0.0"] and got["foreign"][3] == "1.0"
    assert 1.9 < float(got["twice"][6]) < 2.1 and float(got["none"][5]) < 0.5 < float(got["first"][5])
    for r in rrows:
        for x in (r[3], r[5], r[6]):
            assert repr(float(x)) == x
    # --positions: the same events, one row each
    rc, ptext = run_command(rules.RulesEngine(), base + ["--positions", fa])
    prow = [ln.split("\t") for ln in ptext.splitlines()[1:]]
    assert rc == 0 and ptext.splitlines()[0].split("\t") == multisite.POSITION_COLUMNS
    assert len(prow) == sum(int(r[3]) - int(r[2]) + 1 for r in rows)
    # the bytes do not depend on --batch-records
    for n in ("1", "3", "100"):
        rec_n = str(tmp_path / ("rec%s.tsv" % n))
        assert run_command(rules.RulesEngine(), base + ["--batch-records", n, fa, "--records", rec_n])[1] == text
        assert open(rec_n).read() == rtext
        assert run_command(rules.RulesEngine(), base + ["--positions", "--batch-records", n, fa])[1] == ptext


def test_command_motif_order_pairs_and_structure(tmp_path):
    fa, sfa = write_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6, 4, 6), seed=3)
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4, 6), seed=4)
    for argv in (["-p", seq, "-u", fa], ["-q", st, "-u", sfa], ["-p", seq, "-q", st, "-u", fa, sfa]):
        rc, text = run_command(rules.RulesEngine(), argv + ["--all-motifs", "--lambda", "1", "--min-cover", "0.01", "--positions"])
        assert rc == 0
        rows = [ln.split("\t") for ln in text.splitlines()[1:]]
        assert len(rows) > 10
        ids = [i for i, _ in SEQS]
        keys = [(ids.index(r[1]), int(r[0].split("M")[1][0]), int(r[2])) for r in rows]
        assert keys == sorted(keys)                                        # record order, then the file's motif order, then position
        assert len({k[1] for k in keys}) == 3
        for n in ("1", "3"):
            assert run_command(rules.RulesEngine(), argv + ["--all-motifs", "--lambda", "1", "--min-cover", "0.01", "--positions", "--batch-records", n])[1] == text
        first = run_command(rules.RulesEngine(), argv + ["--lambda", "1", "--min-cover", "0.01", "--positions"])[1].splitlines()
        assert first[1:] == [ln for ln, k in zip(text.splitlines()[1:], keys) if k[1] == 0]


def test_option_errors(tmp_path, capsys):
    fa, sfa = write_inputs(tmp_path)
    seq = write_pfm(tmp_path / "seq.pfm", RNA, (6,))
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6,))
    for argv in (["-p", seq, "--prior-sites", "1", "--lambda", "0.1", fa], ["-p", seq, "--prior-sites", "-1", fa], ["-p", seq, "--lambda", "nan", fa],
                 ["-p", seq, "--lambda", "inf", fa], ["-p", seq, "--min-cover", "nan", fa], ["-p", seq, "--batch-records", "0", fa]):
        with pytest.raises(SystemExit) as e:                               # the parser's own refusals
            run_command(None, argv)
        assert e.value.code == 2
    capsys.readouterr()
    for argv, needles in (([fa], ("-p", "-q")), (["-p", seq, fa, sfa], ("-p", "one input")), (["-p", seq, "-q", st, fa], ("two inputs",)),
                          (["-p", seq, "-u", str(tmp_path)], ("averaged-structure", "not supported")),
                          (["-p", seq, "-q", st, "-u", fa, str(tmp_path)], ("averaged-structure", "not supported"))):
        rc, text = run_command(None, argv)
        err = capsys.readouterr().err
        assert rc == 1 and text == ""
        for needle in needles:
            assert needle in err


def test_an_overflowing_partition_function_exits_and_writes_nothing(tmp_path, capsys):
    site = "AAAGGCUCUUUUCAGAGC"
    fa = tmp_path / "repeat.fa"
    fa.write_text(">fine\n%s\n>repeat\n%s\n" % (site + "ACGU" * 5, site * 40))
    rec = tmp_path / "rec.tsv"
    for extra in ([], ["--batch-records", "1"], ["--positions"]):
        rc, text = run_command(rules.RulesEngine(), ["-p", SLBP_PFM, "-u", "-C", "0.01", "--lambda", "1e6", str(fa), "--records", str(rec)] + extra)
        err = capsys.readouterr().err
        assert rc == 1 and text == "" and not rec.exists()                 # nothing is written
        assert "record repeat" in err and "Motif" in err and "smaller" in err and "--prior-sites" in err
    rc, text = run_command(rules.RulesEngine(), ["-p", SLBP_PFM, "-u", "-C", "0.01", str(fa), "--records", str(rec)])
    assert rc == 0 and rec.exists() and len(text.splitlines()) > 2
