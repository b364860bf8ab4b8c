"""`python -m rnascan_amd.footprint` on the GPU: the table equals, byte for byte, what the same `main` writes with the rules
(tests/footprint_rules.py) in the device's place -- for -p, -q and -p with -q, regions and positions, three batch sizes, and a
dot-bracket structure FASTA against its letters file."""
import pytest

import footprint_rules as rules
from conftest import nasty_fasta
from test_footprint_cpu import HIST_FA, SLBP_PFM, run_command
from test_gpu_pair_cli import SLBP_STRUCT_PFM, TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM, structure_files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def both(engine, argv):
    rc, want = run_command(rules.RulesEngine(), argv)
    assert rc == 0 and len(want.splitlines()) >= 2
    assert run_command(engine, argv) == (0, want)
    return want


def test_the_three_input_forms_and_batch_sizes(engine, tmp_path):
    _, letters = structure_files(engine, tmp_path, TEST_FA)
    forms = (["-p", TEST_SEQ_PFM, TEST_FA], ["-q", TEST_STRUCT_PFM, "--struct-format", "letters", letters],
             ["-p", TEST_SEQ_PFM, "-q", TEST_STRUCT_PFM, "--struct-format", "letters", TEST_FA, letters])
    for form in forms:
        for extra in (["-u", "-C", "0.01", "--min-cover", "0.1"], ["-C", "0.01", "--min-cover", "0.2", "--positions"],
                      ["-u", "-C", "0.01", "--weight", "ratio", "--min-cover", "3.5"]):
            want = both(engine, form + extra)
            for n in ("1", "7"):                                      # one record, seven, the default: not a byte changes
                assert run_command(engine, form + extra + ["--batch-records", n]) == (0, want)
    # records of many lengths, some empty, some with foreign letters, some with the SLBP site
    fa = str(tmp_path / "nasty.fa")
    nasty_fasta(fa)
    for extra in ([], ["--positions", "--min-cover", "0.3"]):
        want = both(engine, ["-p", SLBP_PFM, "-u", "-C", "0.01", fa] + extra)
        assert len(want.splitlines()) > 10
        for n in ("1", "7"):
            assert run_command(engine, ["-p", SLBP_PFM, "-u", "-C", "0.01", fa, "--batch-records", n] + extra) == (0, want)


def test_the_slbp_example_prints_its_site(engine, tmp_path):
    want = both(engine, ["-p", SLBP_PFM, "-u", "-C", "0", HIST_FA])
    rows = [ln.split("\t") for ln in want.splitlines()[1:]]
    assert len(rows) == 1 and rows[0][2:4] == ["213", "230"]
    _, letters = structure_files(engine, tmp_path, HIST_FA)
    both(engine, ["-p", SLBP_PFM, "-q", SLBP_STRUCT_PFM, "-C", "0.01", "--struct-format", "letters", HIST_FA, letters])


def test_a_dotbracket_file_is_annotated_first(engine, tmp_path):
    db, letters = structure_files(engine, tmp_path, TEST_FA)
    for base in (["-q", TEST_STRUCT_PFM, "-C", "0.05", "--min-cover", "0.3"], ["-q", TEST_STRUCT_PFM, "-u", "--positions", "--min-cover", "0.3"]):
        want = both(engine, base + ["--struct-format", "letters", letters])
        for argv in (base + ["--struct-format", "dotbracket", db], base + [db], base + ["--batch-records", "4", db]):
            assert run_command(engine, argv) == (0, want)
    pair = ["-p", TEST_SEQ_PFM, "-q", TEST_STRUCT_PFM, "-C", "0.01", "--min-cover", "0.3"]
    want = both(engine, pair + ["--struct-format", "letters", TEST_FA, letters])
    assert run_command(engine, pair + [TEST_FA, db]) == (0, want)
