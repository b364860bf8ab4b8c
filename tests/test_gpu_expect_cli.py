"""`python -m rnascan_amd.expect` on the GPU: the two files equal, byte for byte, what the command writes with the rules
(tests/expect_rules.py) in the device's place -- for -p and -q (letters and dot-bracket), two batch sizes, a multi-PFM file of
two widths and two iterations."""
import os
import shutil

import pytest

from conftest import DATA_DIR
from test_expect_cpu import _RuleEngine, outputs, run_command
from test_gpu_occupancy_cli import DOTBRACKET
from test_occupancy_cpu import STRUCT, write_pfm

pytestmark = pytest.mark.gpu

TEST_FA = os.path.join(DATA_DIR, "test.fa")
TEST_PFM = os.path.join(DATA_DIR, "test_seq_pfm.txt")


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def both(engine, tmp_path, argv, fa):
    """the command on the GPU and with the rules in the device's place: the same bytes in both files"""
    assert run_command(engine, argv + ["-o", str(tmp_path / "gpu"), fa]) == 0
    assert run_command(_RuleEngine(), argv + ["-o", str(tmp_path / "rule"), fa]) == 0
    got = outputs(tmp_path / "gpu")
    assert got == outputs(tmp_path / "rule")
    return got


def test_sequence_fasta_weights_and_batch_sizes(engine, tmp_path):
    for extra in (["-u"], ["--weight", "ratio"], ["--iterations", "2"]):
        base = ["-p", TEST_PFM, "-C", "0.01"] + extra
        got = both(engine, tmp_path, base, TEST_FA)
        assert len(got[1].splitlines()) == (3 if "--iterations" in extra else 2)
        for n in ("1", "7"):                                          # one record, seven: not a byte changes
            assert run_command(engine, base + ["--batch-records", n, "-o", str(tmp_path / "batch"), TEST_FA]) == 0
            assert outputs(tmp_path / "batch") == got


def test_structure_fasta_in_both_forms(engine, tmp_path):
    from rnascan_amd import dotbracket
    db = tmp_path / "db.fa"
    db.write_text("".join(">%s\n%s\n" % rec for rec in DOTBRACKET))
    letters = tmp_path / "letters.fa"
    shutil.move(dotbracket.annotated_copy(engine.ctx, str(db)), letters)
    pfm = write_pfm(tmp_path / "st.pfm", STRUCT, (5, 3, 5), seed=4)
    for extra in (["-u"], ["--all-motifs", "--iterations", "2"]):
        base = ["-q", pfm, "-C", "0.05"] + extra
        got = both(engine, tmp_path, base + ["--struct-format", "letters"], str(letters))
        for argv in (base + ["--struct-format", "dotbracket"], base, base + ["--batch-records", "4"]):   # annotated first, as occupancy -q does
            assert run_command(engine, argv + ["-o", str(tmp_path / "db"), str(db)]) == 0
            assert outputs(tmp_path / "db") == got


def test_all_motifs_of_two_widths(engine, tmp_path):
    pfm = write_pfm(tmp_path / "lib.pfm", "ACGU", (6, 4, 6, 9, 4), seed=8)
    base = ["-p", pfm, "-C", "0.1", "--all-motifs"]
    got = both(engine, tmp_path, base, TEST_FA)
    assert [ln[1:] for ln in got[0].splitlines() if ln.startswith("#M")] == ["M0", "M1", "M2", "M3", "M4"]
    assert run_command(engine, base + ["--batch-records", "7", "-o", str(tmp_path / "b"), TEST_FA]) == 0
    assert outputs(tmp_path / "b") == got
    # every batch staged once and passed to the device once per width, the per-record matrices of all widths kept on the host
    assert run_command(engine, base + ["--merge", "host", "--batch-records", "7", "-o", str(tmp_path / "h"), TEST_FA]) == 0
    assert outputs(tmp_path / "h") == got
    both(engine, tmp_path, base + ["--iterations", "2", "--weight", "ratio"], TEST_FA)
