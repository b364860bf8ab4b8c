"""`python -m rnascan_amd.occupancy` on averaged-structure profiles on the GPU: the bytes equal those of the same command with
the rules in the device's place, in both modes, for a directory and a store, for every batch size, for a library of two
widths; and the default structure background is the one `rnascan -g` prints for the same input."""
import io

import pytest

from test_occupancy_profile_cpu import STRUCT, _RuleEngine, make_inputs, rows_of, write_pfm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("occp")
    fa, d, st, data, order = make_inputs(tmp, lengths=(40, 3, 75, 130, 12, 260, 700, 33, 1, 300, 64), seed=4)
    return dict(tmp=tmp, fa=fa, dir=d, store=st, order=order,
                seq=write_pfm(tmp / "seq.pfm", "ACGU", (6,), seed=2), st=write_pfm(tmp / "st.pfm", STRUCT, (6,), seed=3),
                lib_seq=write_pfm(tmp / "lseq.pfm", "ACGU", (6, 4, 6, 9), seed=5, ids=["A", "B", "C", "D"]),
                lib_st=write_pfm(tmp / "lst.pfm", STRUCT, (6, 4, 6, 9), seed=6, ids=["A", "B", "C", "D"]))


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


@pytest.mark.parametrize("dtype", [None, "float32"])
def test_both_modes_directory_store_and_batch_sizes(engine, inputs, dtype):
    extra = ["-u", "-C", "0.01"] + (["--profile-dtype", dtype] if dtype else [])
    joint = ["-p", inputs["seq"], "-q", inputs["st"]] + extra + [inputs["fa"]]
    text = both(engine, joint + [inputs["dir"]])
    assert [r[1] for r in rows_of(text)] == inputs["order"] and any(float(r[3]) > 0 for r in rows_of(text))
    assert both(engine, joint + [inputs["store"]]) == text                          # directory against store
    for n in ("1", "3", "64"):
        assert run(engine, joint + ["--batch-records", n, inputs["dir"]])[1] == text
        assert run(engine, joint + ["--batch-records", n, inputs["store"]])[1] == text
    only = ["-q", inputs["st"]] + extra
    stored = both(engine, only + [inputs["store"]])
    assert sorted(both(engine, only + [inputs["dir"]]).splitlines()) == sorted(stored.splitlines())
    for n in ("1", "3", "64"):
        assert run(engine, only + ["--batch-records", n, inputs["store"]])[1] == stored
    assert all(int(r[2]) >= int(j[2]) for r, j in zip(sorted(rows_of(stored)), sorted(rows_of(text), key=lambda r: r[1])))


def test_scratch_cap_changes_no_byte(engine, inputs, monkeypatch):
    joint = ["-p", inputs["lib_seq"], "-q", inputs["lib_st"], "--all-motifs", "-u", inputs["fa"], inputs["store"]]
    only = ["-q", inputs["lib_st"], "--all-motifs", "-u", inputs["store"]]
    want = [run(engine, joint)[1], run(engine, only)[1]]
    for cap in ("1", "7", "1000"):
        monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
        assert [run(engine, joint)[1], run(engine, only)[1]] == want


def test_all_motifs_over_two_widths(engine, inputs):
    joint = ["-p", inputs["lib_seq"], "-q", inputs["lib_st"], "--all-motifs", "-u", inputs["fa"]]
    text = both(engine, joint + [inputs["store"]])
    rows = rows_of(text)
    ids = ["A", "B", "C", "D"]
    assert all([r[0] for r in rows[k:k + 4]] == ids for k in range(0, len(rows), 4)) and len(rows) == 4 * len(inputs["order"])
    assert run(engine, joint + ["--batch-records", "2", inputs["dir"]])[1] == text
    only = both(engine, ["-q", inputs["lib_st"], "--all-motifs", "-u", inputs["store"]])
    assert [r[0] for r in rows_of(only)[:4]] == ids
    # a column of the table is the single-motif run of that PFM alone
    alone = write_pfm(inputs["tmp"] / "one.pfm", STRUCT, (6,), seed=6)
    one = rows_of(run(engine, ["-q", alone, "-u", inputs["store"]])[1])
    assert [r[2:] for r in one] == [r[2:] for r in rows_of(only) if r[0] == "A"]


@pytest.mark.parametrize("form", ["dir", "store"])
def test_default_structure_background_is_rnascan_g(engine, inputs, form, capsys):
    """without -u or -B: the bytes of -B with the dict that `rnascan -q .. -g` prints for the same input"""
    from rnascan_amd import cli
    out = io.StringIO()
    with pytest.raises(SystemExit) as e:
        cli.main(["-q", inputs["st"], "-g", inputs[form]], engine=engine, out=out)
    assert not e.value.code and out.getvalue().startswith("{'E': ")
    bg = inputs["tmp"] / ("bg_%s.txt" % form)
    bg.write_text(out.getvalue())
    for argv in (["-q", inputs["st"]], ["-p", inputs["seq"], "-q", inputs["st"], inputs["fa"]]):
        rc, text = run(engine, argv + [inputs[form]])
        assert rc == 0 and text == run(engine, ["-B", str(bg)] + argv + [inputs[form]])[1]
        assert text == run(_RuleEngine(), ["-B", str(bg)] + argv + [inputs[form]])[1]
        assert text != run(engine, ["-u"] + argv + [inputs[form]])[1]
