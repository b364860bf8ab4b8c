"""In-silico mutagenesis without a GPU: the rule against its slow per-variant form, the variants-file parser and its
errors, effect classification, row formatting, and the library's new symbols."""
import io
import os

import numpy as np
import pytest

import mutation_rules as rules
from conftest import assert_f32_bits_equal


@pytest.mark.parametrize("m", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("kind", ["finite", "neginf", "bothinf", "negzero", "halves"])
def test_rule_equals_slow_form(oracle, m, kind):
    rng = np.random.default_rng(100 * m + len(kind))
    T = rules.table(rng, m, kind)
    for lengths, foreign in (([1, max(m - 1, 0), m, m + 1, 2 * m - 1, 2 * m - 2], 0.0), ([23, 9, 20], 0.15), ([m], 0.0)):
        codes = rules.stream(rng, lengths, foreign)
        assert codes.size <= 60
        best, where = rules.mutmap(oracle, codes, T)
        sbest, swhere = rules.mutmap_slow(oracle, codes, T)
        assert_f32_bits_equal(best, sbest)
        assert np.array_equal(where, swhere)
        assert np.all(np.isnan(best[codes >= 4])) and np.all(where[codes >= 4] == -1)


def test_rule_ref_column_is_the_unmutated_best(oracle):
    rng = np.random.default_rng(5)
    m = 4
    T = rules.table(rng, m)
    codes = rules.stream(rng, [30, 7])
    best, where = rules.mutmap(oracle, codes, T)
    sc = oracle.stream_seq(codes, T)
    for p in np.flatnonzero(codes < 4):
        lo, hi = max(0, p - m + 1), min(p, codes.size - m)
        win = sc[lo:hi + 1]
        if np.all(np.isnan(win)):
            assert np.isnan(best[p, codes[p]]) and where[p, codes[p]] == -1
        else:
            k = int(np.nanargmax(win))                      # the first of equal maxima: the lowest start
            assert best[p, codes[p]].view(np.uint32) == win[k].view(np.uint32) and where[p, codes[p]] == p - (lo + k)


def test_rule_ties_go_to_the_lowest_start(oracle):
    T = np.full((2, 8), np.nan)
    T[:, :4] = 1.0                                           # every window scores 2
    codes = np.asarray([0, 1, 2, 3, 7], dtype=np.uint8)
    best, where = rules.mutmap(oracle, codes, T)
    assert np.all(best[:4] == 2.0)
    assert where[:4, 0].tolist() == [0, 1, 1, 1] and np.all(where[4] == -1)


def test_rule_zero_sign_starts_from_plus_zero(oracle):
    T = np.full((1, 8), np.nan)
    T[0, :4] = -0.0
    best, _ = rules.mutmap(oracle, np.asarray([2], dtype=np.uint8), T)
    assert np.all(best.view(np.uint32) == 0)                 # 0.0 + (-0.0) = +0.0


def test_effects():
    from rnascan_amd import variants
    f = np.float32
    thr = float(f(1.5))
    up, down = np.nextafter(f(1.5), f(2)), np.nextafter(f(1.5), f(1))
    ref = np.asarray([np.nan, -np.inf, 1.5, up, down, 2.0, 2.0, np.nan, np.inf], dtype=np.float32)
    alt = np.asarray([2.0, 2.0, up, 1.5, up, np.nan, -np.inf, np.nan, 1.0], dtype=np.float32)
    want = ["gain", "gain", "gain", "loss", "gain", "loss", "loss", "none", "loss"]
    assert [variants.EFFECTS[e] for e in variants.classify(ref, alt, thr)] == want
    assert np.array_equal(variants.classify(ref, alt, thr), rules.effect_codes(ref, alt, thr))
    # thr equal to a score: strict
    assert variants.EFFECTS[int(variants.classify([1.5], [1.5], thr)[0])] == "none"
    assert variants.EFFECTS[int(variants.classify([up], [up], thr)[0])] == "kept"
    # at -inf only NaN / -inf fail
    assert [variants.EFFECTS[e] for e in variants.classify([np.nan, -np.inf, 0.0], [0.0, 0.0, np.nan], -np.inf)] == ["gain", "gain", "loss"]
    assert variants.EFFECTS == rules.EFFECTS


def _write(tmp_path, text):
    p = tmp_path / "v.tsv"
    p.write_text(text)
    return str(p)


def test_parser_reads_header_case_and_t(tmp_path):
    from rnascan_amd import variants
    path = _write(tmp_path, "Seq_ID\tPos\tRef\tAlt\nr1\t3\ta\tT\n\nr2\t1\tU\tg\r\n")
    got = variants.parse_variants(path)
    assert got == [(2, "r1", 2, 0, 3), (4, "r2", 0, 3, 2)]
    rec, start = variants.resolve(path, got, ["r0", "r1", "r2"], [5, 3, 1])
    assert rec.tolist() == [1, 2] and start.tolist() == [2, 0]


@pytest.mark.parametrize("text, line, word", [
    ("r1\t1\tA\tC\nr1\t2\tAC\tG\n", 2, "indels are not supported"),
    ("r1\t1\tA\t-\n", 1, "not a nucleotide"),
    ("Seq_ID\tPos\tRef\tAlt\nr1\t1\tN\tC\n", 2, "not a nucleotide"),
    ("r1\t1\tA\t\n", 1, "indels are not supported"),
    ("r1\tx\tA\tC\n", 1, "not an integer"),
    ("r1\t1\tA\n", 1, "four tab-separated fields"),
])
def test_parser_errors_name_the_line(tmp_path, text, line, word):
    from rnascan_amd import variants
    with pytest.raises(variants.VariantsError) as e:
        variants.parse_variants(_write(tmp_path, text))
    assert e.value.line == line and "line %d" % line in str(e.value) and word in str(e.value)


@pytest.mark.parametrize("text, line, word", [
    ("r1\t1\tA\tC\nnope\t1\tA\tC\n", 2, "unknown Seq_ID"),
    ("r1\t0\tA\tC\n", 1, "outside record"),
    ("r1\t1\tA\tC\nr1\t2\tA\tC\nr1\t4\tA\tC\n", 3, "outside record"),
])
def test_resolve_errors_name_the_line(tmp_path, text, line, word):
    from rnascan_amd import variants
    path = _write(tmp_path, text)
    with pytest.raises(variants.VariantsError) as e:
        variants.resolve(path, variants.parse_variants(path), ["r1"], [3])
    assert e.value.line == line and word in str(e.value)


class _RuleEngine(object):
    """HipEngine's three calls answered by the rule (the CPU stand-in the command's host logic is tested with)"""

    def __init__(self, oracle):
        self.oracle = oracle

    def variants(self, stream, tables, pos, alt):
        tables = np.asarray(tables)
        pos, alt = np.asarray(pos, dtype=np.int64), np.asarray(alt)
        shape = (pos.size, tables.shape[0])
        ref_s, alt_s = np.full(shape, np.nan, np.float32), np.full(shape, np.nan, np.float32)
        ref_w, alt_w = np.full(shape, -1, np.int8), np.full(shape, -1, np.int8)
        for q in range(tables.shape[0]):
            best, where = rules.mutmap(self.oracle, stream.codes, tables[q])
            ok = np.flatnonzero(stream.codes[pos] < 4)
            c = stream.codes[pos[ok]]
            ref_s[ok, q], ref_w[ok, q] = best[pos[ok], c], where[pos[ok], c]
            alt_s[ok, q], alt_w[ok, q] = best[pos[ok], alt[ok]], where[pos[ok], alt[ok]]
        return ref_s, alt_s, ref_w, alt_w

    def mutmap_events(self, stream, table, thr):
        best, _ = rules.mutmap(self.oracle, stream.codes, table)
        return rules.events(stream.codes, best, thr)

    def close(self):
        pass


FASTA = ">r1 first\nACGUACGUAAGGCUCUUUUCAGAGCACGU\n>r2\nacgtnacgtAAAGGCTCTTTTCAGAGCAA\n>r3\nGG\n"


def _pfm(tmp_path, widths=(6,), seed=0):
    rng = np.random.default_rng(seed)
    p = tmp_path / "m.pfm"
    with open(p, "w") as f:
        for k, m in enumerate(widths):
            if len(widths) > 1:
                f.write("#M%d\n#" % k)
            f.write("PO\tA\tC\tG\tU\n")
            for j in range(m):
                f.write("%d\t%s\n" % (j, "\t".join("%.4f" % x for x in rng.dirichlet(np.full(4, 0.4)))))
            f.write("\n")
    return str(p)


def _run(oracle, argv):
    from rnascan_amd import variants
    out = io.StringIO()
    rc = variants.main(argv, engine=_RuleEngine(oracle), out=out)
    return rc, out.getvalue()


def test_rows_format_as_the_scan_does(oracle, tmp_path):
    """every LogOdds cell is what TsvWriter prints for np.round(float32, 3); Delta for the rounded float64 difference"""
    from rnascan_amd import table, variants
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    vf = _write(tmp_path, "Seq_ID\tPos\tRef\tAlt\nr1\t12\tG\tA\nr2\t5\tA\tC\nr1\t1\tA\tU\nr3\t2\tG\tG\nr2\t12\ta\tC\n".replace("r2\t5\tA\tC\n", ""))
    rc, text = _run(oracle, ["-p", _pfm(tmp_path), "-u", "-C", "0.1", "-m", "1", "--variants", vf, str(fa)])
    assert rc == 0
    lines = text.splitlines()
    assert lines[0].split("\t") == variants.COLUMNS and len(lines) == 5
    got = [ln.split("\t") for ln in lines[1:]]
    assert [(g[1], g[2], g[3], g[4]) for g in got] == [("r1", "12", "G", "A"), ("r1", "1", "A", "U"), ("r3", "2", "G", "G"), ("r2", "12", "A", "C")]
    assert got[2][5] == "" and got[2][6] == "" and got[2][9] == "" and got[2][10] == "none"      # a record shorter than the motif
    for g in got[:2] + got[3:]:
        r, a = np.float32(g[6]), np.float32(g[8])
        ref = io.StringIO()
        w = table.TsvWriter(ref, ["x", "y"], match_id=False, header=False)
        w.write_chunk({"x": np.asarray([r, a], dtype=np.float32), "y": np.zeros(2)}, 2)
        w.close()
        assert [ln.split("\t")[0] for ln in ref.getvalue().splitlines()] == [g[6], g[8]]
        assert g[10] in variants.EFFECTS and int(g[5]) >= 1 and int(g[7]) >= 1


def test_command_errors_exit_1_with_the_line(oracle, tmp_path, capsys):
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    pfm = _pfm(tmp_path)
    for text, line, word in (("r1\t1\tC\tG\n", 1, "is not the letter"), ("r1\t1\tA\tG\nr2\t5\tA\tG\n", 2, "is not the letter"),
                             ("r1\t1\tA\tG\nr9\t1\tA\tG\n", 2, "unknown Seq_ID"), ("r3\t3\tG\tA\n", 1, "outside record"),
                             ("r1\t1\tA\tGG\n", 1, "indels are not supported"), ("r1\t1\tA\tN\n", 1, "not a nucleotide")):
        rc, out = _run(oracle, ["-p", pfm, "-u", "--variants", _write(tmp_path, text), str(fa)])
        err = capsys.readouterr().err
        assert rc == 1 and "line %d" % line in err and word in err
        assert out.count("\n") <= 1                          # no row before the error


def test_saturate_and_list_agree_and_do_not_depend_on_batching(oracle, tmp_path, monkeypatch):
    from rnascan_amd import variants
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    pfm = _pfm(tmp_path, widths=(6, 4, 6), seed=3)
    base = ["-p", pfm, "-u", "-C", "0.1", "-m", "2", "--all-motifs"]
    rc, sat = _run(oracle, base + ["--saturate", str(fa)])
    assert rc == 0
    rows = [ln.split("\t") for ln in sat.splitlines()[1:]]
    assert rows and all(r[10] in ("gain", "loss") for r in rows)
    order = {"M0": 0, "M1": 1, "M2": 2}
    keys = [(["r1", "r2", "r3"].index(r[1]), int(r[2]), "ACGU".index(r[4]), order[r[0]]) for r in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    monkeypatch.setattr(variants, "BATCH_RECORDS", 2)
    assert _run(oracle, base + ["--saturate", str(fa)])[1] == sat
    monkeypatch.setattr(variants, "BATCH_RECORDS", 1)
    assert _run(oracle, base + ["--saturate", str(fa)])[1] == sat
    # the list mode on the same events, in another order, prints the same rows
    vf = _write(tmp_path, "".join("%s\t%s\t%s\t%s\n" % (r[1], r[2], r[3], r[4]) for r in reversed(rows)))
    rc, lst = _run(oracle, base + ["--effects-only", "--variants", vf, str(fa)])
    assert rc == 0 and set(lst.splitlines()[1:]) == set(sat.splitlines()[1:])
    full = _run(oracle, base + ["--variants", vf, str(fa)])[1].splitlines()[1:]
    assert len(full) == 3 * len(rows)                        # one row per variant x motif, input order then file order
    assert [ln.split("\t")[0] for ln in full[:3]] == ["M0", "M1", "M2"]
    assert [tuple(ln.split("\t")[1:5]) for ln in full[::3]] == [tuple(r[1:5]) for r in reversed(rows)]


def test_library_exports_the_new_symbols():
    from rnascan_amd import _lib, build
    build.build_lib()
    L = _lib.load()
    assert _lib.ABI_VERSION >= 20 and L.pfmscan_abi_version() == _lib.ABI_VERSION
    for name in ("pfmscan_mutmap_dev", "pfmscan_mutmap_staged", "pfmscan_mutmap_events_dev", "pfmscan_mutmap_events_staged",
                 "pfmscan_variants_dev", "pfmscan_variants_staged"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfmscan.h")).read()
    assert int(re.search(r"#define\s+PFMSCAN_ABI_VERSION\s+(\d+)", text).group(1)) >= 20
