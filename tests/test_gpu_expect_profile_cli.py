"""python -m rnascan_amd.expect_profile on the device against the same command on the rules engine
(tests/test_expect_profile_cpu.py), byte for byte: the three forms, a text directory and a packed store."""
import numpy as np
import pytest

from test_expect_profile_cpu import _RuleEngine, outputs, run_command
from test_occupancy_profile_cpu import STRUCT, make_inputs, write_pfm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


@pytest.mark.parametrize("form", ["struct", "joint", "seq"])
def test_command_on_the_device_equals_the_rules(engine, tmp_path, form):
    fa, d, st, data, order = make_inputs(tmp_path, lengths=(40, 3, 75, 130, 12, 260, 700, 33))
    seq = write_pfm(tmp_path / "seq.pfm", "ACGU", (6, 4), seed=2, ids=["A", "B"])
    stp = write_pfm(tmp_path / "st.pfm", STRUCT, (6, 4), seed=3, ids=["A", "B"])
    opts = (["-p", seq] if form != "struct" else []) + (["-q", stp] if form != "seq" else [])
    with_seq = form != "struct"
    runs = [(["-u", "-C", "0.01", "--all-motifs"], d), (["-u", "-C", "0.01", "--weight", "ratio", "--batch-records", "3"], st),
            (["-C", "0.02", "--iterations", "2", "--profile-dtype", "float32"], st), (["-C", "0.02", "--all-motifs"], d)]
    for extra, source in runs:
        inputs = [source] if form == "struct" else [fa, source]
        assert run_command(engine, opts + extra + ["-o", str(tmp_path / "gpu")] + inputs) == 0
        assert run_command(_RuleEngine(), opts + extra + ["-o", str(tmp_path / "cpu")] + inputs) == 0
        got, want = outputs(tmp_path / "gpu", with_seq), outputs(tmp_path / "cpu", with_seq)
        assert got == want
        assert len(got[0].splitlines()) >= 7 and np.isfinite([float(x) for x in got[0].splitlines()[-2].split("\t")[1:]]).all()
