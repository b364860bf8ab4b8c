"""`python -m rnascan_amd.expect_profile --joint` on the GPU, end to end: on the histone example under tests/golden/data/ and
on a small made-up library, all four files equal, byte for byte, the recorded outputs under tests/golden/expect_profile_joint/
and what the command writes with the rules (tests/expect_profile_joint_rules.py) in the device's place -- on both merge routes
and on ``auto``, with one record per device call, over two iterations and on a directory of two stored column orders."""
import os

import pytest

from test_expect_profile_joint_cpu import LIB_LENGTHS, _RuleEngine, golden, hist_inputs, joint_outputs
from test_expect_profile_cpu import outputs, run_command
from test_occupancy_profile_cpu import FILE_ORDER, STRUCT, make_inputs, write_pfm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


def test_histone_example(engine, tmp_path):
    fa, d, seq, stp = hist_inputs(tmp_path)
    for name, opts in (("hist_joint", ["-p", seq, "-q", stp]), ("hist_seq", ["-p", seq])):
        base = opts + ["-u", "-C", "0", "--joint"]
        want = golden(name)
        assert run_command(_RuleEngine(), base + ["-o", str(tmp_path / "rule"), fa, d]) == 0
        assert joint_outputs(tmp_path / "rule") == want
        for k, extra in enumerate(([], ["--batch-records", "1"], ["--merge", "host"], ["--merge", "device"], ["--merge", "auto"])):
            assert run_command(engine, base + extra + ["-o", str(tmp_path / ("gpu%d" % k)), fa, d]) == 0
            assert joint_outputs(tmp_path / ("gpu%d" % k)) == want, extra
        # without --joint: the other files have the same bytes, and no table is written
        assert run_command(engine, [o for o in base if o != "--joint"] + ["-o", str(tmp_path / "plain"), fa, d]) == 0
        assert outputs(tmp_path / "plain") == want[:3] and not os.path.exists(str(tmp_path / "plain") + ".expected.joint.txt")
        assert len(want[3].splitlines()) >= 2 and want[3].split("\t", 2)[:2] == ["PO", "A.B"]


def test_made_up_library_iterations_and_column_orders(engine, tmp_path):
    fa, d, st, data, order = make_inputs(tmp_path, lengths=LIB_LENGTHS)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4, 6), seed=2, ids=["A", "B", "C"])
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4, 6), seed=3, ids=["A", "B", "C"])
    base = ["-p", seq, "-q", stp, "-u", "-C", "0.01", "--all-motifs", "--joint"]
    want = golden("library")
    runs = ((["--merge", "device"], d), (["--merge", "host"], st), (["--batch-records", "1"], d), (["--batch-records", "3", "--weight", "posterior"], st))
    for k, (extra, source) in enumerate(runs):
        assert run_command(engine, base + extra + ["-o", str(tmp_path / ("gpu%d" % k)), fa, source]) == 0
        assert joint_outputs(tmp_path / ("gpu%d" % k)) == want, extra
    rows = [ln.split("\t")[:2] for ln in want[3].splitlines()]
    assert rows == [["Motif", "PO"]] + [[mid, str(k)] for mid, m in (("A", 6), ("B", 4), ("C", 6)) for k in range(m)]
    assert run_command(engine, [o for o in base if o != "--joint"] + ["-o", str(tmp_path / "plain"), fa, d]) == 0
    assert outputs(tmp_path / "plain") == want[:3]
    # --iterations 2: a run on the outputs of a run; the table is the last pass's
    it = ["-p", seq, "-q", stp, "-C", "0.02", "--all-motifs", "--joint", "--weight", "ratio"]
    assert golden("two") != want
    for merge in ("device", "host"):
        assert run_command(engine, it + ["--iterations", "2", "--merge", merge, "-o", str(tmp_path / "two"), fa, st]) == 0
        assert joint_outputs(tmp_path / "two") == golden("two")
    assert run_command(engine, it + ["-o", str(tmp_path / "first"), fa, st]) == 0
    first = str(tmp_path / "first")
    assert run_command(engine, ["-p", first + ".expected.seq.txt", "-q", first + ".expected.struct.txt"] + it[4:] + ["-o", str(tmp_path / "second"), fa, st]) == 0
    two, second = golden("two"), joint_outputs(tmp_path / "second")
    assert two[0] == second[0] and two[2:] == second[2:]


def test_two_stored_column_orders(engine, tmp_path):
    """every run of equal stored order is mapped to the profile's letters before the records are added.  With -p alone no sum
    runs over the columns: the bytes are those of the same data stored in one order.  With -q the marginal adds in the stored
    order, so the bytes are the rules' on the same directory (and only close to the one-order run's)"""
    other = "EHTBLRM"
    orders = [FILE_ORDER, other, other, FILE_ORDER, other, FILE_ORDER, other, other]
    fa, mixed, _, data, order = make_inputs(tmp_path, lengths=LIB_LENGTHS, orders=orders, name="mixed")
    (tmp_path / "one").mkdir()
    _, plain, _, _, _ = make_inputs(tmp_path / "one", lengths=LIB_LENGTHS)
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6,), seed=2)
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6,), seed=3)
    for merge in ("device", "host"):
        tail = ["-u", "-C", "0.01", "--joint", "--merge", merge, "--batch-records", "3"]
        assert run_command(engine, ["-p", seq] + tail + ["-o", str(tmp_path / "m"), fa, mixed]) == 0
        assert run_command(engine, ["-p", seq] + tail + ["-o", str(tmp_path / "p"), fa, plain]) == 0
        assert joint_outputs(tmp_path / "m") == joint_outputs(tmp_path / "p")
        assert run_command(engine, ["-p", seq, "-q", stp] + tail + ["-o", str(tmp_path / "m"), fa, mixed]) == 0
        assert run_command(_RuleEngine(), ["-p", seq, "-q", stp] + tail[:-4] + ["-o", str(tmp_path / "r"), fa, mixed]) == 0
        assert joint_outputs(tmp_path / "m") == joint_outputs(tmp_path / "r")
