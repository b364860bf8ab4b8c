"""`python -m rnascan_amd.occupancy` on the GPU: the rows equal the rules' values formatted by the same rule, the bytes do
not depend on the batch size, structure input in both forms, and a multi-PFM file of two widths keeps its motif order."""
import io
import os
import shutil

import numpy as np
import pytest

from conftest import DATA_DIR
from test_occupancy_cpu import STRUCT, _RuleEngine, write_pfm

pytestmark = pytest.mark.gpu

TEST_FA = os.path.join(DATA_DIR, "test.fa")
TEST_PFM = os.path.join(DATA_DIR, "test_seq_pfm.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "test_struct_pfm.txt")
DOTBRACKET = [("s1 hairpin", "((((...))))..((..)).."), ("s2", "...."), ("s3", "(((..(((...)))..)))...((((....))))."),
              ("s4", "." * 40 + "(((((" + "." * 7 + ")))))" + "." * 25), ("s5", "((...))"), ("s6", "((..((...))..((...))..))")]


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def run(engine, argv):
    from rnascan_amd import occupancy
    out = io.StringIO()
    rc = occupancy.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def both(engine, argv):
    """the command on the GPU and with the rules in the device's place: the same bytes"""
    rc, text = run(engine, argv)
    assert rc == 0
    assert text == run(_RuleEngine(), argv)[1]
    return text


def test_example_fasta_and_batch_sizes(engine):
    from rnascan_amd import occupancy
    with open(TEST_FA) as f:
        n_rec = sum(1 for ln in f if ln.startswith(">"))
    for bg in (["-u"], []):                                       # uniform, and computed from the input as rnascan does
        base = ["-p", TEST_PFM, "-C", "0.01"] + bg
        text = both(engine, base + [TEST_FA])
        lines = text.splitlines()
        assert lines[0].split("\t") == occupancy.COLUMNS and len(lines) == 1 + n_rec
        assert all(ln.split("\t")[0] == "test_seq_pfm" for ln in lines[1:])
        assert any(float(ln.split("\t")[3]) > 0 for ln in lines[1:])
        for n in ("1", "7", str(n_rec)):                          # one record, seven, everything: not a byte changes
            assert run(engine, base + ["--batch-records", n, TEST_FA])[1] == text


def test_structure_fasta_in_both_forms(engine, tmp_path):
    from rnascan_amd import dotbracket
    db = tmp_path / "db.fa"
    db.write_text("".join(">%s\n%s\n" % rec for rec in DOTBRACKET))
    tmp = dotbracket.annotated_copy(engine.ctx, str(db))
    letters = tmp_path / "letters.fa"
    shutil.move(tmp, letters)
    body = "".join(ln for ln in letters.read_text().splitlines() if not ln.startswith(">"))
    assert set(body) <= set(STRUCT + STRUCT.lower()) and len(body) == sum(len(s) for _, s in DOTBRACKET)
    pfm = write_pfm(tmp_path / "st.pfm", STRUCT, (5, 3, 5), seed=4, zero=True)
    for extra in (["-u"], [], ["--all-motifs"]):
        base = ["-q", pfm, "-C", "0.05"] + extra
        text = both(engine, base + ["--struct-format", "letters", str(letters)])
        assert run(engine, base + ["--struct-format", "dotbracket", str(db)])[1] == text      # annotated first, as rnascan -q does
        assert run(engine, base + [str(db)])[1] == text                                       # auto
        for n in ("1", "4"):
            assert run(engine, base + ["--batch-records", n, str(db)])[1] == text
    text = both(engine, ["-q", STRUCT_PFM, "-u", "-C", "0.01", "--struct-format", "letters", str(letters)])
    assert len(text.splitlines()) == 1 + len(DOTBRACKET)


def test_all_motifs_of_two_widths_keep_the_file_order(engine, tmp_path):
    pfm = write_pfm(tmp_path / "lib.pfm", "ACGU", (6, 4, 6, 9, 4), seed=8)
    base = ["-p", pfm, "-C", "0.1", "--all-motifs"]
    text = both(engine, base + [TEST_FA])
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    ids = ["M0", "M1", "M2", "M3", "M4"]
    assert [r[0] for r in rows[:5]] == ids and all([r[0] for r in rows[k:k + 5]] == ids for k in range(0, len(rows), 5))
    assert len(set(r[1] for r in rows[:5])) == 1 and rows[0][1] != rows[5][1]                  # record order, then motif order
    for n in ("1", "7"):
        assert run(engine, base + ["--batch-records", n, TEST_FA])[1] == text
    # a column of the table is the single-motif run of that PFM alone
    alone = write_pfm(tmp_path / "one.pfm", "ACGU", (6,), seed=8)
    one = run(engine, ["-p", alone, "-C", "0.1", TEST_FA])[1].splitlines()[1:]
    assert [ln.split("\t")[2:] for ln in one] == [r[2:] for r in rows if r[0] == "M0"]
