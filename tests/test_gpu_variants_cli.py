"""`python -m rnascan_amd.variants` on the GPU: the example inputs, the scan of an actually mutated FASTA, input order,
batching, awkward FASTA files and parser errors."""
import io
import os

import pytest

from conftest import DATA_DIR, nasty_fasta
from test_mutation_cpu import FASTA, _RuleEngine, _pfm

pytestmark = pytest.mark.gpu

SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
SITE = "AAAGGCTCTTTTCAGAGC"                       # the SLBP site of the example record


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def run(engine, argv):
    from rnascan_amd import variants
    out = io.StringIO()
    rc = variants.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def hist_sequence():
    with open(HIST_FA) as f:
        lines = f.read().splitlines()
    return lines[0], "".join(lines[1:])


def test_saturate_on_the_example_and_scan_of_the_mutated_fasta(engine, oracle, tmp_path):
    from rnascan_amd import cli
    base = ["-p", SEQ_PFM, "-u", "-C", "0.01", "-m", "10"]
    rc, text = run(engine, base + ["--saturate", HIST_FA])
    assert rc == 0
    assert text == run(_RuleEngine(oracle), base + ["--saturate", HIST_FA])[1]          # every row, scores and starts: the rule's
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    header, seq = hist_sequence()
    site = seq.find(SITE)
    assert site >= 0
    inside = [r for r in rows if r[10] == "loss" and site < int(r[2]) <= site + len(SITE)]
    assert inside and all(r[10] in ("gain", "loss") for r in rows)
    # the letter actually changed, scanned by rnascan at -m ' -inf': the LogOdds at Alt.Start is this table's Alt.LogOdds
    for k, r in enumerate((inside + rows)[:5]):
        p = int(r[2]) - 1
        assert seq[p].upper().replace("T", "U") == r[3]
        fa = tmp_path / ("mut%d.fa" % k)
        fa.write_text(header + "\n" + seq[:p] + r[4] + seq[p + 1:] + "\n")
        out = io.StringIO()
        cli.main(["-p", SEQ_PFM, "-u", "-C", "0.01", "-m", " -inf", str(fa)], engine=engine, out=out)
        table = [ln.split("\t") for ln in out.getvalue().splitlines()]
        start, logodds = table[0].index("Start"), table[0].index("LogOdds")
        hit = [t for t in table[1:] if t[start] == r[7]]
        assert len(hit) == 1 and hit[0][logodds] == r[8]


def test_list_keeps_input_order_and_batching_changes_no_byte(engine, oracle, tmp_path, monkeypatch):
    from rnascan_amd import variants
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    pfm = _pfm(tmp_path, widths=(6, 4, 6), seed=3)
    vf = tmp_path / "v.tsv"
    vf.write_text("Seq_ID\tPos\tRef\tAlt\nr2\t12\ta\tC\nr1\t12\tG\tA\nr3\t2\tG\tU\nr1\t1\tA\tt\nr2\t12\tA\tC\nr1\t29\tU\tG\n")
    base = ["-p", pfm, "-u", "-C", "0.1", "-m", "2", "--all-motifs"]
    rc, lst = run(engine, base + ["--variants", str(vf), str(fa)])
    assert rc == 0
    got = [ln.split("\t") for ln in lst.splitlines()[1:]]
    assert [g[0] for g in got] == ["M0", "M1", "M2"] * 6
    assert [(g[1], g[2], g[4]) for g in got[::3]] == [("r2", "12", "C"), ("r1", "12", "A"), ("r3", "2", "U"), ("r1", "1", "U"), ("r2", "12", "C"), ("r1", "29", "G")]
    rc, sat = run(engine, base + ["--saturate", str(fa)])
    assert rc == 0 and len(sat.splitlines()) > 1
    rule = _RuleEngine(oracle)
    assert lst == run(rule, base + ["--variants", str(vf), str(fa)])[1] and sat == run(rule, base + ["--saturate", str(fa)])[1]
    for size in (2, 1 << 30):
        monkeypatch.setattr(variants, "BATCH_RECORDS", size)
        assert run(engine, base + ["--variants", str(vf), str(fa)])[1] == lst
        assert run(engine, base + ["--saturate", str(fa)])[1] == sat
    only = run(engine, base + ["--effects-only", "--variants", str(vf), str(fa)])[1].splitlines()[1:]
    assert only == [ln for ln in lst.splitlines()[1:] if ln.split("\t")[10] in ("gain", "loss")]


def test_nasty_fasta(engine, oracle, tmp_path, monkeypatch):
    from rnascan_amd import variants
    fa = str(tmp_path / "nasty.fa")
    nasty_fasta(fa, n=24)
    base = ["-p", SEQ_PFM, "-u", "-C", "0.01", "-m", "8"]
    rc, sat = run(engine, base + ["--saturate", fa])
    rows = [ln.split("\t") for ln in sat.splitlines()[1:]]
    assert rc == 0 and any(r[10] == "loss" for r in rows)
    assert sat == run(_RuleEngine(oracle), base + ["--saturate", fa])[1]
    monkeypatch.setattr(variants, "BATCH_RECORDS", 2)
    assert run(engine, base + ["--saturate", fa])[1] == sat
    vf = tmp_path / "v.tsv"                                       # the events as a list: the same rows
    vf.write_text("".join("%s\t%s\t%s\t%s\n" % (r[1], r[2], r[3].replace("U", "t"), r[4]) for r in rows[:40]))
    rc, lst = run(engine, base + ["--variants", str(vf), fa])
    assert rc == 0 and lst.splitlines()[1:] == sat.splitlines()[1:41]


@pytest.mark.parametrize("text, line, word", [
    ("r1\t1\tC\tG\n", 1, "is not the letter"),
    ("Seq_ID\tPos\tRef\tAlt\nr1\t1\tA\tG\nr2\t5\tA\tG\n", 3, "is not the letter"),
    ("r1\t1\tA\tG\nr9\t1\tA\tG\n", 2, "unknown Seq_ID"),
    ("r3\t3\tG\tA\n", 1, "outside record"),
    ("r1\t1\tA\tGG\n", 1, "indels are not supported"),
    ("r1\t1\tA\tN\n", 1, "not a nucleotide"),
])
def test_parser_errors_exit_1(engine, tmp_path, capsys, text, line, word):
    fa = tmp_path / "s.fa"
    fa.write_text(FASTA)
    vf = tmp_path / "v.tsv"
    vf.write_text(text)
    rc, out = run(engine, ["-p", _pfm(tmp_path), "-u", "--variants", str(vf), str(fa)])
    err = capsys.readouterr().err
    assert rc == 1 and "line %d" % line in err and word in err and out.count("\n") <= 1
