"""`python -m rnascan_amd.multisite_profile` on the GPU: the bytes (the table and --records) equal those of the same command with
the rules in the device's place, on the reference's example record structure only and joint, and for a library run with
--all-motifs at two batch sizes."""
import io

import pytest

import multisite_profile_rules as rules
from test_multisite_profile_cpu import HIST_FA, SLBP_SEQ, SLBP_STRUCT, hist_dir
from test_occupancy_profile_cpu import STRUCT, make_inputs, write_pfm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def run(engine, argv, records):
    from rnascan_amd import multisite_profile
    out = io.StringIO()
    rc = multisite_profile.main(argv + ["--records", str(records)], engine=engine, out=out)
    return rc, out.getvalue(), open(str(records)).read() if rc == 0 else None


def both(engine, argv, tmp):
    """the command on the GPU and with the rules in the device's place: the same bytes, --records too"""
    got = run(engine, argv, tmp / "gpu.tsv")
    assert got[0] == 0
    assert got == run(rules.RulesEngine(), argv, tmp / "rules.tsv")
    return got[1], got[2]


def test_the_example_record(engine, tmp_path):
    d, sid = hist_dir(tmp_path)
    base = ["-u", "-C", "0", "--pairing", "aligned"]
    text, recs = both(engine, ["-p", SLBP_SEQ, "-q", SLBP_STRUCT, "--prior-sites", "0.01"] + base + [HIST_FA, d], tmp_path)
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    assert len(rows) == 1 and rows[0][1] == sid and rows[0][2:4] == ["213", "230"]
    assert len(recs.splitlines()) == 2 and 5.75e12 < float(recs.splitlines()[1].split("\t")[3]) < 5.77e12
    text, recs = both(engine, ["-q", SLBP_STRUCT] + base + [d], tmp_path)           # the structure PFM alone: several regions
    assert len(text.splitlines()) > 3 and 2.4e33 < float(recs.splitlines()[1].split("\t")[3]) < 2.6e33
    both(engine, ["-q", SLBP_STRUCT, "--positions", "--profile-dtype", "float32"] + base + [d], tmp_path)


def test_a_library_with_all_motifs_and_two_batch_sizes(engine, tmp_path):
    fa, d, st, data, order = make_inputs(tmp_path, lengths=(40, 3, 75, 130, 12, 260, 700, 33, 1, 300, 64), seed=4)
    lib_seq = write_pfm(tmp_path / "lseq.pfm", "ACGU", (6, 4, 6, 9), seed=5, ids=["A", "B", "C", "D"])
    lib_st = write_pfm(tmp_path / "lst.pfm", STRUCT, (6, 4, 6, 9), seed=6, ids=["A", "B", "C", "D"])
    extra = ["--all-motifs", "-u", "-C", "0.01", "--min-cover", "0.05"]
    joint = ["-p", lib_seq, "-q", lib_st] + extra + [fa]
    text, recs = both(engine, joint + [d], tmp_path)
    assert len(text.splitlines()) > 20 and len(recs.splitlines()) == 1 + 11 * 4
    assert both(engine, joint + [st], tmp_path) == (text, recs)                      # directory against store
    for n in ("1", "3"):
        got = run(engine, joint + ["--batch-records", n, d], tmp_path / "b.tsv")
        assert got == (0, text, recs)
    stored = both(engine, ["-q", lib_st] + extra + ["--positions", st], tmp_path)
    assert run(engine, ["-q", lib_st] + extra + ["--positions", "--batch-records", "3", st], tmp_path / "b.tsv") == (0,) + stored
