"""Per-record column sums of averaged-structure profiles on the device (pfmscan_profile_colsums_*) against the numpy
restatement of their order of additions (tests/background_rules.py), BIT FOR BIT; the invariance of the background under
batching, chunking, upload mode, input form and ranks; rejections; the command line."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import background_rules as rules
from average_rules import PAIRS, golden, golden_fasta_path, split_name
from background_helpers import COLUMNS, RulesEngine, random_rows, write_fasta, write_profile
from conftest import DATA_DIR, REPO

pytestmark = pytest.mark.gpu

SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(engine):
    return engine.ctx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev_sums(ctx, st):
    """pfmscan_profile_colsums_dev on torch buffers"""
    import torch
    dev = torch.device("cuda", 0)
    prof = torch.from_numpy(np.ascontiguousarray(st.profile)).to(dev)
    off = torch.from_numpy(np.ascontiguousarray(st.offsets)).to(dev)
    ln = torch.from_numpy(np.ascontiguousarray(st.lengths)).to(dev)
    out = torch.full((len(st.offsets), 7), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.profile_colsums_dev(prof.data_ptr() if prof.numel() else None, st.profile.dtype, st.profile.shape[0], off.data_ptr(),
                            ln.data_ptr(), len(st.offsets), out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


def all_three(engine, st):
    """(_host, _host in small chunks, _staged, _dev)"""
    ctx = engine.ctx
    host = ctx.profile_colsums_host(st.profile, st.offsets, st.lengths)
    os.environ["PFMSCAN_COLSUMS_CHUNK"] = "3000"
    try:
        chunked = ctx.profile_colsums_host(st.profile, st.offsets, st.lengths)
    finally:
        del os.environ["PFMSCAN_COLSUMS_CHUNK"]
    ctx.stage(None, st.profile)
    staged = ctx.profile_colsums_staged(st.offsets, st.lengths)
    return host, chunked, staged, dev_sums(ctx, st)


def check(engine, profs, dtype):
    from rnascan_amd import pack
    st = pack.pack(profiles=profs, profile_dtype=dtype)
    want = rules.colsums(st.profile, st.offsets, st.lengths)
    for name, got in zip(("host", "chunked", "staged", "dev"), all_three(engine, st)):
        assert got.shape == want.shape, name
        assert np.array_equal(bits(got), bits(want)), (name, np.flatnonzero((bits(got) != bits(want)).any(axis=1))[:5])
    return st, want


# ---- 4. bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sums_equal_the_restatement_bit_for_bit(engine, dtype):
    rng = np.random.default_rng(3)
    P = rules.PIECE
    lengths = [0, 1, 2, 3, 4, 5, 63, 64, 65, P - 1, P, P + 1, 3 * P + 700, 0, 0, 255, 256, 257, 3000]
    lengths += list(range(0, 70)) + list(range(70, 0, -1))         # records starting at every residue of the row mod 4 and mod 64
    profs = [(rng.random((L, 7)) * rng.choice([1.0, 1e-7, 1e4])).astype(dtype) for L in lengths]
    st, _ = check(engine, profs, dtype)
    assert {int(o) % 4 for o in st.offsets} == {0, 1, 2, 3} and len({int(o) % 64 for o in st.offsets}) == 64
    check(engine, [rng.random((5 * P + 11, 7)).astype(dtype)], dtype)             # one record only
    check(engine, [rng.random((1, 7)).astype(dtype)], dtype)
    check(engine, [np.zeros((0, 7), dtype=dtype)], dtype)                         # ... and an empty one


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_hundred_thousand_short_records(engine, dtype):
    rng = np.random.default_rng(4)
    lengths = rng.integers(0, 40, size=100000)
    rows = rng.random((int(lengths.sum()), 7)).astype(dtype)
    cuts = np.concatenate([[0], np.cumsum(lengths)])
    check(engine, [rows[cuts[i]:cuts[i + 1]] for i in range(lengths.size)], dtype)


@pytest.mark.parametrize("w,o", PAIRS)
def test_golden_average_profiles(engine, w, o):
    from rnascan_amd import _lib
    profs = [_lib.profile_parse(body, 7) for _, body in sorted(golden(w, o)[2].items())]
    assert len(profs) > 3
    check(engine, profs, np.float64)
    check(engine, profs, np.float32)


def test_stream_longer_than_2_31_rows(ctx):
    """float32 rows generated on the device, cells multiples of 1/1024: the expected sums are exact integers over 1024"""
    import torch
    if torch.cuda.mem_get_info()[0] < 80e9:
        pytest.skip("needs 80 GB of free HBM")
    dev = torch.device("cuda", 0)
    L, per = 3000, 20000                                            # records of 3000 rows + separator, generated 20000 at a time
    n_rec = ((1 << 31) + 5000000) // (L + 1) // per * per + per
    n_pos = n_rec * (L + 1)
    assert n_pos > (1 << 31)
    prof = torch.empty((n_pos, 7), dtype=torch.float32, device=dev)
    want = torch.empty((n_rec, 7), dtype=torch.int64, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    for r0 in range(0, n_rec, per):
        ints = torch.randint(0, 1025, (per, L + 1, 7), dtype=torch.int32, device=dev, generator=g)
        ints[:, L, :] = 0
        want[r0:r0 + per] = ints.sum(dim=1, dtype=torch.int64)
        prof[r0 * (L + 1):(r0 + per) * (L + 1)] = (ints.to(torch.float32) / 1024).reshape(-1, 7)
        del ints
    off = torch.arange(n_rec, dtype=torch.int64, device=dev) * (L + 1)
    ln = torch.full((n_rec,), L, dtype=torch.int64, device=dev)
    out = torch.empty((n_rec, 7), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.profile_colsums_dev(prof.data_ptr(), np.float32, n_pos, off.data_ptr(), ln.data_ptr(), n_rec, out.data_ptr())
    ctx.synchronize()
    assert bool(torch.equal(out * 1024, want.to(torch.float64)))
    # a bad cell beyond the 2^31st row is named by its 64-bit element index
    row = n_pos - 2
    prof[row, 3] = float("nan")
    torch.cuda.synchronize()
    with pytest.raises(ValueError) as e:
        ctx.profile_colsums_dev(prof.data_ptr(), np.float32, n_pos, off.data_ptr(), ln.data_ptr(), n_rec, out.data_ptr())
    assert e.value.element == row * 7 + 3
    del prof, want, out
    torch.cuda.empty_cache()


# ---- 6. rejections -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rejections_name_the_earliest_cell(engine, dtype):
    from rnascan_amd import pack
    rng = np.random.default_rng(8)
    P = rules.PIECE
    lengths = [300, 2 * P + 123, 1, 50]
    base = pack.pack(profiles=[rng.random((L, 7)).astype(dtype) for L in lengths], profile_dtype=dtype)
    off = [int(x) for x in base.offsets]
    last = off[3] + 49
    cases = [[(0, 0, np.nan)], [(last, 6, -1.0)], [(off[0] + 299, 2, np.inf)], [(off[1], 5, -np.inf)],      # first / last row, beside separators
             [(off[1] + 2 * P + 100, 4, np.nan)],                                                                # the last piece of a long record
             [(off[2], 1, -1e-30)], [(off[1] + P + 7, 3, np.nan), (off[0] + 17, 6, -2.0), (last, 0, np.inf)]]    # several: the earliest wins
    for cells in cases:
        prof = base.profile.copy()
        for row, col, val in cells:
            prof[row, col] = val
        st = pack.Stream(None, prof, base.offsets, base.lengths)
        want = min(row * 7 + col for row, col, _ in cells)
        assert rules.first_bad(prof, st.offsets, st.lengths) == want
        ctx = engine.ctx
        calls = [lambda: ctx.profile_colsums_host(st.profile, st.offsets, st.lengths),
                 lambda: (ctx.stage(None, st.profile), ctx.profile_colsums_staged(st.offsets, st.lengths)),
                 lambda: dev_sums(ctx, st), lambda: engine.profile_colsums(st)]
        for call in calls:
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.element == want, cells
        os.environ["PFMSCAN_COLSUMS_CHUNK"] = "1000"
        try:
            with pytest.raises(ValueError) as e:
                calls[0]()
        finally:
            del os.environ["PFMSCAN_COLSUMS_CHUNK"]
        assert e.value.element == want, cells
    # a bad value in a SEPARATOR row belongs to no record; the sums are those of the clean stream
    prof = base.profile.copy()
    prof[off[0] + 300, 2] = np.nan
    got = engine.ctx.profile_colsums_host(prof, base.offsets, base.lengths)
    assert np.array_equal(bits(got), bits(rules.colsums(base.profile, base.offsets, base.lengths)))
    # a table that does not describe the stream is refused, whatever it holds
    with pytest.raises(ValueError):
        engine.ctx.profile_colsums_host(base.profile, base.offsets, base.lengths + 1)
    st = pack.Stream(None, base.profile, base.offsets, base.lengths + 1)
    with pytest.raises(ValueError):
        dev_sums(engine.ctx, st)


# ---- 5. invariance -----------------------------------------------------------------------------------------------------
def _dict_bits(d):
    return [(k, float(v).hex()) for k, v in d.items()]


def test_background_does_not_depend_on_how_the_work_was_cut(engine, tmp_path, monkeypatch):
    from rnascan_amd import background, scanner, store
    rng = np.random.default_rng(12)
    lengths = rng.integers(2000, 4000, size=650)                    # 55 MB of float32 rows: the staged uploader takes part
    n_pos = int(lengths.sum() + lengths.size)
    sdir = str(tmp_path / "store")
    os.makedirs(sdir)
    rows = np.zeros((n_pos, 7), dtype=np.float32)
    at = 0
    for L in lengths:
        rows[at:at + L] = rng.dirichlet(np.ones(7), size=int(L)).astype(np.float32)
        at += int(L) + 1
    rows.tofile(os.path.join(sdir, "profile.f32"))
    store.write_index(sdir, ["r%d" % i for i in range(lengths.size)], [int(x) for x in lengths], list(COLUMNS), np.float32, "profile.f32")
    ps = store.ProfileStore(sdir)
    st = ps.stream()
    want = rules.content(rules.colsums(st.profile, st.offsets, st.lengths), COLUMNS)
    seen = []
    for batch in ("5000", "300000", str(1 << 24)):
        for upload in ("0", "1"):
            for chunk in (None, "70000"):
                monkeypatch.setenv("RNASCAN_BATCH_POSITIONS", batch)
                monkeypatch.setenv("PFMSCAN_UPLOAD", upload)
                if chunk:
                    monkeypatch.setenv("PFMSCAN_COLSUMS_CHUNK", chunk)
                else:
                    monkeypatch.delenv("PFMSCAN_COLSUMS_CHUNK", raising=False)
                seen.append(_dict_bits(background.profile_background(engine, sdir, verbose=False)))
    monkeypatch.delenv("PFMSCAN_UPLOAD")
    monkeypatch.delenv("PFMSCAN_COLSUMS_CHUNK", raising=False)
    monkeypatch.delenv("RNASCAN_BATCH_POSITIONS")
    assert all(s == _dict_bits(want) for s in seen)
    # a staged stream is summed where it lies
    engine._stage(st)
    assert np.array_equal(bits(engine.profile_colsums(st)), bits(rules.colsums(st.profile, st.offsets, st.lengths)))
    # text directory and store of the same values
    d = tmp_path / "avg"
    d.mkdir()
    profs = [random_rows(rng, int(L)) for L in rng.integers(1, 900, size=40)]
    for i, p in enumerate(profs):
        write_profile(str(d / ("structure.t%d.txt" % i)), p)
    s64, s32 = str(tmp_path / "s64"), str(tmp_path / "s32")
    store.build_store(str(d), s64, np.float64)
    store.build_store(str(d), s32, np.float32)                      # multiples of 1/1024 are float32 numbers
    got = [_dict_bits(background.profile_background(engine, src, verbose=False)) for src in (str(d), s64, s32)]
    monkeypatch.setenv("RNASCAN_BATCH_POSITIONS", "700")
    got.append(_dict_bits(background.profile_background(engine, str(d), verbose=False)))
    assert got[0] == got[1] == got[2] == got[3]
    assert got[0] == _dict_bits(background.profile_background(RulesEngine(), str(d), verbose=False))


def _clean_env(**extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra)
    return env


@pytest.fixture()
def inputs(tmp_path):
    """sequence FASTA, averaged-structure directory, float64 store of the same 60 records"""
    from rnascan_amd import store
    rng = np.random.default_rng(33)
    d = tmp_path / "avg"
    d.mkdir()
    recs = []
    for i in range(60):
        L = int(rng.integers(20, 400))
        recs.append(("q%02d" % i, "".join(rng.choice(list("ACGU"), size=L))))
        write_profile(str(d / ("structure.q%02d.txt" % i)), random_rows(rng, L))
    fa = str(tmp_path / "seqs.fa")
    write_fasta(fa, recs)
    sdir = str(tmp_path / "store")
    store.build_store(str(d), sdir, np.float64)
    return {"fa": fa, "dir": str(d), "store": sdir}


@pytest.mark.timeout(600)
def test_two_ranks_print_what_one_rank_prints(inputs):
    exe = [sys.executable, os.path.join(REPO, "bin", "rnascan")]
    for argv in (["-q", STRUCT_PFM, "-C", "0.01", "-m", "-60", inputs["store"]], ["-q", STRUCT_PFM, "-g", inputs["store"]],
                 ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.01", "-m", "-60", inputs["fa"], inputs["store"]],
                 ["-q", STRUCT_PFM, "-g", inputs["dir"]]):
        one = subprocess.run(exe + argv, env=_clean_env(), capture_output=True, text=True, timeout=280)
        assert one.returncode == 0, one.stderr[-3000:]
        two = subprocess.run(exe + argv + ["--gpus", "2"], env=_clean_env(RNASCAN_ONE_DEVICE="1"), capture_output=True, text=True,
                             timeout=280)
        assert two.returncode == 0, two.stderr[-3000:]
        assert one.stdout.count("\n") >= 1 and two.stdout == one.stdout, argv


@pytest.mark.timeout(600)
def test_two_ranks_reject_the_earliest_cell(inputs, tmp_path):
    """a bad cell in the second rank's share and an earlier one in the first's: exit 1, no stdout, the first one's message"""
    from rnascan_amd import fasta, store
    for rid, row, letter, cell in (("q52", 3, "M", "nan"), ("q05", 7, "H", "-0.5")):
        path = os.path.join(inputs["dir"], "structure.%s.txt" % rid)
        _, prof = fasta.read_profile(path)
        rows = [[repr(x) for x in r] for r in prof.tolist()]
        rows[row][COLUMNS.index(letter)] = cell
        write_profile(path, rows)
    sdir = str(tmp_path / "badstore")
    store.build_store(inputs["dir"], sdir, np.float64)
    exe = [sys.executable, os.path.join(REPO, "bin", "rnascan")]
    for argv in (["-q", STRUCT_PFM, sdir], ["-p", SEQ_PFM, "-q", STRUCT_PFM, inputs["fa"], sdir], ["-q", STRUCT_PFM, "-g", sdir]):
        for extra, env in (([], _clean_env()), (["--gpus", "2"], _clean_env(RNASCAN_ONE_DEVICE="1"))):
            r = subprocess.run(exe + argv + extra, env=env, capture_output=True, text=True, timeout=280)
            assert r.returncode == 1, (argv, extra, r.returncode, r.stderr[-3000:])
            assert r.stdout == ""
            assert "q05" in r.stderr and "position 8" in r.stderr and "column H" in r.stderr, r.stderr[-3000:]
            assert "Traceback" not in r.stderr and "q52" not in r.stderr, r.stderr[-3000:]


# ---- 7. the command line -----------------------------------------------------------------------------------------------
def _run(argv, engine, code=None):
    from rnascan_amd import cli
    out = io.StringIO()
    if code is None:
        cli.main(argv, engine=engine, out=out)
    else:
        with pytest.raises(SystemExit) as e:
            cli.main(argv, engine=engine, out=out)
        assert (e.value.code or 0) == code
    return out.getvalue()


def _rows(t):
    return sorted("\t".join(l.split("\t")[:-1]) for l in t.split("\n")[1:] if l)


def _same_table(got, want):
    """the same rows; the unrounded fp64 structure scores within the 1e-6 the engine keeps to the oracle"""
    g, w = _rows(got), _rows(want)
    assert len(g) == len(w) and len(g) > 5
    for a, b in zip(g, w):
        a, b = a.split("\t"), b.split("\t")
        for x, y in zip(a, b):
            if x != y:
                assert abs(float(x) - float(y)) <= 1e-6, (a, b)


def test_cli_on_the_device_against_the_oracle_backed_engine(engine, inputs, tmp_path, capsys):
    for src in ("dir", "store"):
        ss = ["-q", STRUCT_PFM, "-C", "0.01", "-m", "-60", inputs[src]]
        rnass = ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.01", "-m", "-60", inputs["fa"], inputs[src]]
        printed = _run(["-q", STRUCT_PFM, "-g", inputs[src]], engine, code=0)
        assert printed == _run(["-q", STRUCT_PFM, "-g", inputs[src]], RulesEngine(), code=0) and printed.startswith("{'E': ")
        bg = tmp_path / ("bg_%s.txt" % src)
        bg.write_text(printed)
        for argv in (ss, rnass):
            capsys.readouterr()
            got = _run(argv, engine)
            assert printed.strip() in capsys.readouterr().err
            _same_table(got, _run(argv, RulesEngine()))
            n = 2 if argv is rnass else 1
            assert got == _run(argv[:-n] + ["-B", str(bg)] + argv[-n:], engine)      # the printed dict fed back: the same hits
    # a rejected cell: exit 1 before any table, the record, position and letter named
    from rnascan_amd import fasta
    path = os.path.join(inputs["dir"], "structure.q07.txt")
    _, prof = fasta.read_profile(path)
    rows = [[repr(x) for x in row] for row in prof.tolist()]
    rows[len(rows) - 1][COLUMNS.index("T")] = "nan"
    write_profile(path, rows)
    capsys.readouterr()
    assert _run(["-q", STRUCT_PFM, inputs["dir"]], engine, code=1) == ""
    err = capsys.readouterr().err
    assert "q07" in err and "position %d" % len(rows) in err and "column T" in err
    assert _run(["-q", STRUCT_PFM, "-u", "-m", "-60", inputs["dir"]], engine).startswith("Sequence_ID")


def test_cli_fragments_take_their_background_from_the_averaged_profiles(engine, tmp_path, capsys):
    from rnascan_amd import average
    w, o = 100, 95
    seqs, frags, _ = golden(w, o)
    fa = golden_fasta_path(tmp_path, w, o)
    have = {split_name(n)[0] for n, _ in frags}
    sq = str(tmp_path / "seqs.fa")
    write_fasta(sq, [(rid, s) for rid, s in seqs if rid in have])
    sdir = str(tmp_path / "avgstore")
    average.build(engine.ctx, fa, sdir, out_fmt="store")
    printed = _run(["-q", STRUCT_PFM, "-g", sdir], engine, code=0)
    assert printed == _run(["-q", STRUCT_PFM, "-g", sdir], RulesEngine(), code=0)
    assert printed == _run(["-q", STRUCT_PFM, "-g", "--struct-format", "fragments", fa], engine, code=0)
    for argv, tail in ((["-q", STRUCT_PFM, "-C", "0.01", "-m", "-30"], []), (["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.01", "-m", "-30"], [sq])):
        want = _run(argv + tail + [sdir], engine)
        assert want.count("\n") > 20
        assert _run(argv + ["--struct-format", "fragments"] + tail + [fa], engine) == want
