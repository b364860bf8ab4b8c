"""`python -m rnascan_amd.footprint_profile` on the GPU: the bytes equal those of the same command with the rules in the
device's place, in both modes, for a directory and a store, for regions and positions and every batch size; and the
reference's example record has its known SLBP site at 213..230 under the structure PFM alone and under both."""
import io

import pytest

import footprint_profile_rules as rules
from test_footprint_profile_cpu import HIST_FA, SLBP_SEQ, SLBP_STRUCT, hist_dir
from test_occupancy_profile_cpu import STRUCT, make_inputs, write_pfm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fpp")
    fa, d, st, data, order = make_inputs(tmp, lengths=(40, 3, 75, 130, 12, 260, 700, 33, 1, 300, 64), seed=4)
    return dict(tmp=tmp, fa=fa, dir=d, store=st, order=order,
                lib_seq=write_pfm(tmp / "lseq.pfm", "ACGU", (6, 4, 6, 9), seed=5, ids=["A", "B", "C", "D"]),
                lib_st=write_pfm(tmp / "lst.pfm", STRUCT, (6, 4, 6, 9), seed=6, ids=["A", "B", "C", "D"]))


def run(engine, argv):
    from rnascan_amd import footprint_profile
    out = io.StringIO()
    rc = footprint_profile.main(argv, engine=engine, out=out)
    return rc, out.getvalue()


def both(engine, argv):
    """the command on the GPU and with the rules in the device's place: the same bytes"""
    rc, text = run(engine, argv)
    assert rc == 0
    assert text == run(rules.RulesEngine(), argv)[1]
    return text


@pytest.mark.parametrize("dtype", [None, "float32"])
@pytest.mark.parametrize("weight", ["posterior", "ratio"])
def test_both_modes_directory_store_positions_and_batch_sizes(engine, inputs, weight, dtype):
    extra = ["--all-motifs", "-u", "-C", "0.01", "--weight", weight, "--min-cover", "0.05" if weight == "posterior" else "2.0"]
    extra += ["--profile-dtype", dtype] if dtype else []
    joint = ["-p", inputs["lib_seq"], "-q", inputs["lib_st"]] + extra + [inputs["fa"]]
    only = ["-q", inputs["lib_st"]] + extra
    for positions in ([], ["--positions"]):
        text = both(engine, joint + positions + [inputs["dir"]])
        assert len(text.splitlines()) > 20
        assert both(engine, joint + positions + [inputs["store"]]) == text          # directory against store
        stored = both(engine, only + positions + [inputs["store"]])
        assert sorted(both(engine, only + positions + [inputs["dir"]]).splitlines()) == sorted(stored.splitlines())
        for n in ("1", "3"):
            assert run(engine, joint + positions + ["--batch-records", n, inputs["dir"]])[1] == text
            assert run(engine, only + positions + ["--batch-records", n, inputs["store"]])[1] == stored


def test_the_known_slbp_site(engine, tmp_path):
    d, sid = hist_dir(tmp_path)
    for argv in (["-q", SLBP_STRUCT, "-u", "-C", "0", "--pairing", "aligned", d],
                 ["-p", SLBP_SEQ, "-q", SLBP_STRUCT, "-u", "-C", "0", "--pairing", "aligned", HIST_FA, d]):
        rows = [ln.split("\t") for ln in both(engine, argv).splitlines()[1:]]
        assert len(rows) == 1 and rows[0][1] == sid and rows[0][2:4] == ["213", "230"]
