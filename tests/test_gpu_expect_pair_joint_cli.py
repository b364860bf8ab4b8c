"""`python -m rnascan_amd.expect_pair --joint` on the GPU, end to end on the inputs under tests/golden/data/: all four files
equal, byte for byte, what the command writes with the rules (tests/pair_joint_rules.py) in the device's place -- on both merge
routes and on ``auto``, with one record per device call, on a dot-bracket structure file, over two iterations and for a
two-motif library."""
import pytest

from test_gpu_pair_cli import HIST_FA, SLBP_SEQ_PFM, SLBP_STRUCT_PFM, TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM, engine, structure_files  # noqa: F401
from test_occupancy_cpu import STRUCT, write_pfm
from test_pair_cpu import run_expect
from test_pair_joint_cpu import _RuleEngine, joint_outputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fa,seq_pfm,struct_pfm", [(TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM), (HIST_FA, SLBP_SEQ_PFM, SLBP_STRUCT_PFM)])
def test_merge_routes_batches_and_dot_bracket_write_the_same_four_files(engine, tmp_path, fa, seq_pfm, struct_pfm):
    db, letters = structure_files(engine, tmp_path, fa)
    for extra in (["-u"], ["--weight", "ratio", "--iterations", "2"]):
        base = ["-p", seq_pfm, "-q", struct_pfm, "-C", "0.01", "--joint"] + extra
        assert run_expect(_RuleEngine(), base + ["--struct-format", "letters", "-o", str(tmp_path / "rule"), fa, letters]) == 0
        want = joint_outputs(tmp_path / "rule")
        assert len(want[3].splitlines()) >= 2 and want[3].split("\t", 2)[:2] == ["PO", "A.B"]
        runs = [["--merge", merge, "--struct-format", "letters", fa, letters] for merge in ("device", "host", "auto")]
        runs += [["--batch-records", "1", "--merge", "device", "--struct-format", "letters", fa, letters], ["--batch-records", "1", "--merge", "host", fa, db], [fa, db]]
        for k, tail in enumerate(runs):
            assert run_expect(engine, base + tail[:-2] + ["-o", str(tmp_path / ("gpu%d" % k))] + tail[-2:]) == 0
            assert joint_outputs(tmp_path / ("gpu%d" % k)) == want, tail


def test_all_motifs_blocks_are_in_pair_order(engine, tmp_path):
    db, letters = structure_files(engine, tmp_path, HIST_FA)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 9, 6), seed=8)
    st = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 9, 6), seed=9)
    base = ["-p", seq, "-q", st, "-C", "0.1", "--all-motifs", "--joint"]
    assert run_expect(_RuleEngine(), base + ["--struct-format", "letters", "-o", str(tmp_path / "rule"), HIST_FA, letters]) == 0
    want = joint_outputs(tmp_path / "rule")
    for merge in ("device", "host"):
        assert run_expect(engine, base + ["--merge", merge, "-o", str(tmp_path / merge), HIST_FA, db]) == 0
        assert joint_outputs(tmp_path / merge) == want
    rows = [ln.split("\t")[:2] for ln in want[3].splitlines()]
    assert rows == [["Motif", "PO"]] + [["M0", str(k)] for k in range(6)] + [["M1", str(k)] for k in range(9)] + [["M2", str(k)] for k in range(6)]
