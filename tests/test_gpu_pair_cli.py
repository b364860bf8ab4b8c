"""`python -m rnascan_amd.occupancy_pair` and `python -m rnascan_amd.expect_pair` on the GPU, end to end on the inputs under
tests/golden/data/: the bytes equal what the commands write with the rules (tests/pair_rules.py) in the device's place --
structure letters and a dot-bracket structure file, two batch sizes, two iterations, and --all-motifs on a two-motif library."""
import os
import shutil

import pytest

from conftest import DATA_DIR
from test_occupancy_cpu import STRUCT, write_pfm
from test_pair_cpu import _RuleEngine, outputs, run_expect, run_occupancy

pytestmark = pytest.mark.gpu

TEST_FA = os.path.join(DATA_DIR, "test.fa")
TEST_SEQ_PFM = os.path.join(DATA_DIR, "test_seq_pfm.txt")
TEST_STRUCT_PFM = os.path.join(DATA_DIR, "test_struct_pfm.txt")
HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
SLBP_SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
SLBP_STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def dotbracket_for(fa, path):
    """a dot-bracket file for the records of a FASTA: nested stems with a bulge around hairpin loops, of every record's length"""
    from rnascan_amd import fasta
    recs = fasta.open_lazy(fa)
    with open(path, "w") as f:
        for sid, n in zip(recs.ids, recs.lengths):
            n, s = int(n), ""
            while n - len(s) >= 16:
                s += "((.((....)).)).."
            f.write(">%s\n%s\n" % (sid, s + "." * (n - len(s))))
    return str(path)


def structure_files(engine, tmp_path, fa):
    """(the dot-bracket file, its annotation as a structure-letter file) for the records of fa"""
    from rnascan_amd import dotbracket
    db = dotbracket_for(fa, tmp_path / (os.path.basename(fa) + ".db"))
    letters = str(tmp_path / (os.path.basename(fa) + ".letters"))
    shutil.move(dotbracket.annotated_copy(engine.ctx, db), letters)
    body = "".join(ln for ln in open(letters).read().splitlines() if not ln.startswith(">"))
    assert set(body) <= set(STRUCT + STRUCT.lower()) and len(set(body.upper())) >= 3
    return db, letters


@pytest.mark.parametrize("fa,seq_pfm,struct_pfm", [(TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM), (HIST_FA, SLBP_SEQ_PFM, SLBP_STRUCT_PFM)])
def test_occupancy_pair_on_the_golden_inputs(engine, tmp_path, fa, seq_pfm, struct_pfm):
    db, letters = structure_files(engine, tmp_path, fa)
    for extra in (["-u"], []):
        base = ["-p", seq_pfm, "-q", struct_pfm, "-C", "0.01"] + extra
        rc, want = run_occupancy(_RuleEngine(), base + ["--struct-format", "letters", fa, letters])
        assert rc == 0 and len(want.splitlines()) >= 2
        for argv in (base + ["--struct-format", "letters", fa, letters], base + [fa, db], base + ["--struct-format", "dotbracket", "--batch-records", "1", fa, db]):
            assert run_occupancy(engine, argv) == (0, want)
    assert float(want.splitlines()[1].split("\t")[3]) > 0


@pytest.mark.parametrize("fa,seq_pfm,struct_pfm", [(TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM), (HIST_FA, SLBP_SEQ_PFM, SLBP_STRUCT_PFM)])
def test_expect_pair_on_the_golden_inputs(engine, tmp_path, fa, seq_pfm, struct_pfm):
    db, letters = structure_files(engine, tmp_path, fa)
    for extra in (["-u"], ["--weight", "ratio"], ["--iterations", "2"]):
        base = ["-p", seq_pfm, "-q", struct_pfm, "-C", "0.01"] + extra
        assert run_expect(_RuleEngine(), base + ["--struct-format", "letters", "-o", str(tmp_path / "rule"), fa, letters]) == 0
        want = outputs(tmp_path / "rule")
        assert len(want[2].splitlines()) == (3 if "--iterations" in extra else 2)
        for k, argv in enumerate((base + ["--struct-format", "letters", fa, letters], base + [fa, db], base + ["--batch-records", "1", fa, db])):
            assert run_expect(engine, argv[:-2] + ["-o", str(tmp_path / ("gpu%d" % k))] + argv[-2:]) == 0
            assert outputs(tmp_path / ("gpu%d" % k)) == want


def test_all_motifs_on_a_two_motif_library(engine, tmp_path):
    db, letters = structure_files(engine, tmp_path, HIST_FA)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 9), seed=8)
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 9), seed=9)
    base = ["-p", seq, "-q", st, "-C", "0.1", "--all-motifs"]
    rc, want = run_occupancy(_RuleEngine(), base + ["--struct-format", "letters", HIST_FA, letters])
    assert rc == 0 and [ln.split("\t")[0] for ln in want.splitlines()[1:]] == ["M0", "M1"]
    assert run_occupancy(engine, base + [HIST_FA, db]) == (0, want)
    for extra in ([], ["--iterations", "2", "--weight", "ratio"]):
        assert run_expect(_RuleEngine(), base + extra + ["--struct-format", "letters", "-o", str(tmp_path / "rule"), HIST_FA, letters]) == 0
        assert run_expect(engine, base + extra + ["-o", str(tmp_path / "gpu"), HIST_FA, db]) == 0
        got = outputs(tmp_path / "gpu")
        assert got == outputs(tmp_path / "rule")
        assert [ln[1:] for ln in got[0].splitlines() if ln.startswith("#M")] == ["M0", "M1"] == [ln[1:] for ln in got[1].splitlines() if ln.startswith("#M")]
