"""`python -m rnascan_amd.multisite` on the GPU: the rows and the --records table equal, byte for byte, what the same `main`
writes with the rules (tests/multisite_rules.py) in the device's place -- for -p, -q and -p with -q, regions and positions, and
a run of several batches against a run of one."""
import pytest

import multisite_rules as rules
from conftest import nasty_fasta
from test_gpu_pair_cli import TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM, structure_files
from test_multisite_cpu import HIST_FA, SLBP_PFM, run_command

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def with_records(engine, argv, path):
    rc, text = run_command(engine, argv + ["--records", str(path)])
    return rc, text, open(str(path)).read() if rc == 0 else None


def both(engine, argv, tmp_path):
    want = with_records(rules.RulesEngine(), argv, tmp_path / "want.tsv")
    assert want[0] == 0 and len(want[2].splitlines()) >= 2
    assert with_records(engine, argv, tmp_path / "got.tsv") == want
    return want


def test_the_slbp_example_rows_and_records(engine, tmp_path):
    base = ["-p", SLBP_PFM, "-u", "-C", "0", HIST_FA]
    want = both(engine, base, tmp_path)
    rows = [ln.split("\t") for ln in want[1].splitlines()[1:]]
    assert len(rows) == 1 and rows[0][2:4] == ["213", "230"]
    assert both(engine, base + ["--prior-sites", "0.01"], tmp_path)[1].splitlines()[1:] == []   # unbound: no region
    both(engine, base + ["--positions", "--lambda", "0.001"], tmp_path)


def test_the_three_input_forms_and_batches(engine, tmp_path):
    _, letters = structure_files(engine, tmp_path, TEST_FA)
    forms = (["-p", TEST_SEQ_PFM, TEST_FA], ["-q", TEST_STRUCT_PFM, "--struct-format", "letters", letters],
             ["-p", TEST_SEQ_PFM, "-q", TEST_STRUCT_PFM, "--struct-format", "letters", TEST_FA, letters])
    for form in forms:
        for extra in (["-u", "-C", "0.01", "--min-cover", "0.1"], ["-C", "0.01", "--min-cover", "0.05", "--positions", "--lambda", "0.5"]):
            want = both(engine, form + extra, tmp_path)
            assert with_records(engine, form + extra + ["--batch-records", "7"], tmp_path / "seven.tsv") == want
    # records of many lengths, some empty, some with foreign letters, some with the SLBP site: two batches against one
    fa = str(tmp_path / "nasty.fa")
    nasty_fasta(fa)
    n_rec = sum(1 for ln in open(fa) if ln.startswith(">"))
    argv = ["-p", SLBP_PFM, "-u", "-C", "0.01", fa]
    want = both(engine, argv, tmp_path)
    assert len(want[1].splitlines()) > 5
    assert with_records(engine, argv + ["--batch-records", str((n_rec + 1) // 2)], tmp_path / "two.tsv") == want
