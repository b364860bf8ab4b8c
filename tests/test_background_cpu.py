"""Structure background of averaged-structure profiles on a GPU-less host: the restated order of additions against
math.fsum, the tie to compute_background (one-hot profiles), and the command line with the oracle-backed engine whose
``profile_colsums`` is the numpy restatement (tests/background_rules.py)."""
import io
import math
import os

import numpy as np
import pytest

import background_rules as rules
from background_helpers import COLUMNS, RulesEngine, as_ranks, one_hot, random_rows, write_fasta, write_profile
from conftest import DATA_DIR
from rnascan_amd import background, cli, fasta, pack, store

SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")

# ---- 1. the restated order against math.fsum -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rules_within_the_textbook_bound_of_fsum(dtype):
    rng = np.random.default_rng(11)
    lengths = [0, 1, 2, 63, 64, 65, 255, 256, 257, rules.PIECE - 1, rules.PIECE, rules.PIECE + 1, 3 * rules.PIECE + 77, 3000]
    profs = [(rng.random((L, 7)) * rng.choice([1.0, 1e-6, 1e3])).astype(dtype) for L in lengths]
    st = pack.pack(profiles=profs, profile_dtype=dtype)
    sums = rules.colsums(st.profile, st.offsets, st.lengths)
    for r, p in enumerate(profs):
        d = rules.depth([lengths[r]])
        assert np.array_equal(sums[r], rules.record_sums(p))
        for c in range(7):
            exact = math.fsum(p[:, c].astype(np.float64).tolist())
            assert abs(sums[r, c] - exact) <= d * 2.0 ** -53 * exact, (lengths[r], c)
    assert rules.depth([3 * rules.PIECE + 77]) == 8 + 6 + 3 + 3
    assert rules.depth([0]) == 0 and rules.depth([1]) == 1 + 6 + 3


# ---- 2. the tie to compute_background ------------------------------------------------------------------------------------
def test_one_hot_profiles_give_compute_background_exactly(tmp_path):
    rng = np.random.default_rng(5)
    lengths = [40, 0, 1, 300, rules.PIECE + 452, 77]
    strings = ["".join(rng.choice(list("EHTBLR"), size=L)) for L in lengths]          # M never occurs
    fa = str(tmp_path / "structs.fa")
    write_fasta(fa, [("r%d" % i, s) for i, s in enumerate(strings)])
    with pytest.warns(Warning):
        want = fasta.compute_background(fa, fasta.STRUCT, verbose=False)
    st = pack.pack(profiles=[one_hot(s) for s in strings], profile_dtype=np.float64)
    eng = RulesEngine()
    with pytest.warns(Warning):
        got = background.content_from_sums(eng.profile_colsums(st), COLUMNS, verbose=False)
    assert list(got.items()) == list(want.items())
    assert list(got) == list(fasta.STRUCT)
    # the same through a text directory and a packed store, columns in another order (matched by NAME)
    d = tmp_path / "avg"
    d.mkdir()
    other = "TRMLHEB"
    kept = [(i, s) for i, s in enumerate(strings) if s]
    for i, s in kept:
        write_profile(str(d / ("structure.r%d.txt" % i)), one_hot(s, other), other)
    fa2 = str(tmp_path / "kept.fa")
    write_fasta(fa2, [("r%d" % i, s) for i, s in kept])
    with pytest.warns(Warning):
        want2 = fasta.compute_background(fa2, fasta.STRUCT, verbose=False)
        got_dir = background.profile_background(eng, str(d), verbose=False)
        sdir = str(tmp_path / "store")
        store.build_store(str(d), sdir, np.float32)
        got_store = background.profile_background(eng, sdir, verbose=False)
    assert list(got_dir.items()) == list(want2.items()) == list(got_store.items())


def test_multiples_of_1024th_are_exact_and_per_record_sums_are_exposed(tmp_path):
    rng = np.random.default_rng(6)
    lengths = [5, 2500, 64, 1]
    profs = [random_rows(rng, L) for L in lengths]
    d = tmp_path / "avg"
    d.mkdir()
    for i, p in enumerate(profs):
        write_profile(str(d / ("structure.s%d.txt" % i)), p)
    ids, letters, sums = background.record_sums(RulesEngine(), str(d))
    assert list(letters) == list(COLUMNS) and sums.shape == (4, 7)
    for sid, row in zip(ids, sums):
        p = profs[int(sid[1:])]
        assert np.array_equal(row * 1024, np.round(p * 1024).sum(axis=0))            # exact integers over 1024
        assert row.sum() == p.shape[0]
    count = {c: sum(int(round(p[:, COLUMNS.index(c)].sum() * 1024)) for p in profs) for c in fasta.STRUCT}
    total = 7 * 1024 + sum(count.values())
    got = background.content_from_sums(sums, letters, verbose=False)
    assert got == {c: (count[c] / 1024 + 1) / (total / 1024) for c in fasta.STRUCT}


# ---- 3. the command line ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def inputs(tmp_path):
    """a sequence FASTA, the averaged-structure directory of the same records, its packed store, the expected dict"""
    rng = np.random.default_rng(21)
    d = tmp_path / "avg"
    d.mkdir()
    recs = []
    for i, L in enumerate([60, 35, 120, 24]):
        recs.append(("q%d" % i, "".join(rng.choice(list("ACGU"), size=L))))
        write_profile(str(d / ("structure.q%d.txt" % i)), random_rows(rng, L))
    fa = str(tmp_path / "seqs.fa")
    write_fasta(fa, recs)
    parsed = [fasta.read_profile(str(d / ("structure.%s.txt" % rid))) for rid, _ in recs]
    st = pack.pack(profiles=[p for _, p in parsed], profile_dtype=np.float64)
    want = rules.content(rules.colsums(st.profile, st.offsets, st.lengths), parsed[0][0])
    bgfile = str(tmp_path / "bg_struct.txt")
    with open(bgfile, "w") as f:
        f.write(repr(want))
    sdir = str(tmp_path / "store")
    store.build_store(str(d), sdir, np.float64)
    return {"fa": fa, "dir": str(d), "store": sdir, "want": want, "bgfile": bgfile}


def run(argv):
    out = io.StringIO()
    cli.main(argv, engine=RulesEngine(), out=out)
    return out.getvalue()


@pytest.mark.parametrize("form", ["dir", "store"])
def test_cli_default_background_equals_the_dict_fed_back(inputs, form, capsys):
    ss = ["-q", STRUCT_PFM, "-C", "0.01", "-m", "-60", inputs[form]]
    got = run(ss)
    err = capsys.readouterr().err
    assert "Calculating background probabilities..." in err and repr(inputs["want"]) in err
    assert got == run(ss[:-1] + ["-B", inputs["bgfile"], inputs[form]])
    assert got.count("\n") > 5
    rnass = ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.01", "-m", "-60", inputs["fa"], inputs[form]]
    got = run(rnass)
    assert got == run(rnass[:-2] + ["-B", inputs["bgfile"], inputs["fa"], inputs[form]])
    assert got.count("\n") > 5


@pytest.mark.parametrize("form", ["dir", "store"])
def test_cli_bgonly_prints_the_dict(inputs, form):
    out = io.StringIO()
    with pytest.raises(SystemExit) as e:
        cli.main(["-q", STRUCT_PFM, "-g", inputs[form]], engine=RulesEngine(), out=out)
    assert not e.value.code
    assert out.getvalue() == repr(inputs["want"]) + "\n"


@pytest.mark.parametrize("cell", ["nan", "inf", "-0.25"])
def test_cli_rejects_a_cell_without_a_background(inputs, cell, capsys):
    path = os.path.join(inputs["dir"], "structure.q2.txt")
    _, prof = fasta.read_profile(path)
    rows = [[repr(x) for x in row] for row in prof.tolist()]
    rows[16][COLUMNS.index("L")] = cell
    rows[90][COLUMNS.index("B")] = "nan"              # a later bad cell of the same record: the earliest wins
    write_profile(path, rows)
    for argv in (["-q", STRUCT_PFM, inputs["dir"]], ["-p", SEQ_PFM, "-q", STRUCT_PFM, inputs["fa"], inputs["dir"]],
                 ["-q", STRUCT_PFM, "-g", inputs["dir"]]):
        out = io.StringIO()
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            cli.main(argv, engine=RulesEngine(), out=out)
        assert e.value.code == 1
        assert out.getvalue() == ""
        err = capsys.readouterr().err
        assert "q2" in err and "position 17" in err and "column L" in err
    # -u and -B do not compute a background: the scan keeps accepting such cells
    assert run(["-q", STRUCT_PFM, "-u", "-m", "-60", inputs["dir"]]).startswith("Sequence_ID")


# ---- 4. several ranks ------------------------------------------------------------------------------------------------------
def test_background_error_survives_the_hand_over_between_ranks():
    import pickle
    e = pickle.loads(pickle.dumps((background.BackgroundError("q2", 17, "L", float("nan")), None)))[0]
    assert isinstance(e, background.BackgroundError)
    assert (e.record, e.position, e.letter) == ("q2", 17, "L") and math.isnan(e.value)
    assert "q2" in str(e) and "position 17" in str(e) and "column L" in str(e)


def _mixed_store(tmp_path, cells=()):
    """a float64 store of 12 records; ``cells`` = (record, row, column letter, value) written into it"""
    rng = np.random.default_rng(31)
    d = tmp_path / "avg12"
    d.mkdir()
    for i in range(12):
        rows = [[repr(x) for x in row] for row in random_rows(rng, 30 + 7 * i).tolist()]
        for rec, row, letter, value in cells:
            if rec == i:
                rows[row][COLUMNS.index(letter)] = value
        write_profile(str(d / ("structure.k%02d.txt" % i)), rows)
    sdir = str(tmp_path / "store12")
    store.build_store(str(d), sdir, np.float64)
    return str(d), sdir


def test_two_and_three_ranks_build_the_dict_of_one_rank(tmp_path):
    d, sdir = _mixed_store(tmp_path)
    for src in (d, sdir):
        one = background.profile_background(RulesEngine(), src, verbose=False)
        for world in (2, 3):
            got = as_ranks(world, lambda r, w, dist: background.profile_background(RulesEngine(), src, r, w, dist, verbose=False))
            assert all(isinstance(g, dict) and [(k, v.hex()) for k, v in g.items()] == [(k, v.hex()) for k, v in one.items()]
                       for g in got), got


def test_every_rank_raises_the_earliest_rejection(tmp_path):
    """a bad cell in the last rank's share and an earlier one in the first's: every rank gets the first one's message"""
    _, sdir = _mixed_store(tmp_path, [(10, 3, "M", "nan"), (1, 5, "H", "-0.5"), (1, 20, "B", "inf")])
    for world in (2, 3):
        got = as_ranks(world, lambda r, w, dist: background.profile_background(RulesEngine(), sdir, r, w, dist, verbose=False))
        for e in got:
            assert isinstance(e, background.BackgroundError), e
            assert (e.record, e.position, e.letter, e.value) == ("k01", 6, "H", -0.5)
    # only the last share is bad: the first rank learns of it too
    (tmp_path / "b").mkdir()
    _, sdir = _mixed_store(tmp_path / "b", [(11, 0, "E", "inf")])
    got = as_ranks(2, lambda r, w, dist: background.profile_background(RulesEngine(), sdir, r, w, dist, verbose=False))
    assert all(isinstance(e, background.BackgroundError) and e.record == "k11" and e.position == 1 for e in got), got


def test_any_failure_of_one_rank_reaches_every_rank(tmp_path):
    class Broken(RulesEngine):
        def profile_colsums(self, stream):
            raise RuntimeError("device lost")
    _, sdir = _mixed_store(tmp_path)
    got = as_ranks(2, lambda r, w, dist: background.record_sums(Broken() if r == 1 else RulesEngine(), sdir, r, w, dist))
    assert all(isinstance(e, RuntimeError) and "device lost" in str(e) for e in got), got


# ---- 5. files of one directory with different column orders ----------------------------------------------------------------------
def test_files_with_their_own_column_orders_are_matched_by_name(tmp_path, capsys):
    rng = np.random.default_rng(41)
    d1, d2 = tmp_path / "same", tmp_path / "mixed"
    d1.mkdir()
    d2.mkdir()
    orders = ["BEHLMRT", "TRMLHEB", "EHTBLRM", "BEHLMRT", "MBTEHLR"]
    for i, order in enumerate(orders):
        p = random_rows(rng, 20 + 11 * i)
        write_profile(str(d1 / ("structure.f%d.txt" % i)), p)
        write_profile(str(d2 / ("structure.f%d.txt" % i)), p[:, [COLUMNS.index(c) for c in order]], order)
    want = background.profile_background(RulesEngine(), str(d1), verbose=False)
    assert background.profile_background(RulesEngine(), str(d2), verbose=False) == want
    got = as_ranks(2, lambda r, w, dist: background.profile_background(RulesEngine(), str(d2), r, w, dist, verbose=False))
    assert got == [want, want]
    # a rejected cell is named by the letter of ITS file's column
    p = [[repr(x) for x in row] for row in random_rows(rng, 9).tolist()]
    p[4][2] = "nan"
    write_profile(str(d2 / "structure.f9.txt"), p, "MBTEHLR")
    with pytest.raises(background.BackgroundError) as e:
        background.profile_background(RulesEngine(), str(d2), verbose=False)
    assert (e.value.record, e.value.position, e.value.letter) == ("f9", 5, "T")
    # columns that are not the seven letters: a clean exit 1 that names the file, no traceback
    write_profile(str(d2 / "structure.f9.txt"), random_rows(rng, 9), "BEHLMRX")
    out = io.StringIO()
    capsys.readouterr()
    with pytest.raises(SystemExit) as x:
        cli.main(["-q", STRUCT_PFM, str(d2)], engine=RulesEngine(), out=out)
    assert x.value.code == 1 and out.getvalue() == "" and "structure.f9.txt" in capsys.readouterr().err
