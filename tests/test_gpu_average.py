"""Fragment averaging on the device (csrc/pfmscan_average.hip behind rnascan_amd.average): the reference's profile texts
(tests/golden/average/), random fragment sets against the numpy restatement (tests/average_rules.py) bit for bit in both
dtypes, a fragment stream longer than 2^31 letters, every rejection with its message, the staged rows, and the command
line on fragments against the same scan of the built text directory and store."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from average_rules import COLUMNS, PAIRS, counts, golden, golden_fasta_path, py2_starts, scanned, split_name
from conftest import DATA_DIR, REPO
from dotbracket_rules import annotate, random_structure

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


def _read_dir(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


# ---- 1. the reference's texts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,o", PAIRS)
def test_build_text_and_store_equal_the_reference(ctx, tmp_path, w, o):
    from rnascan_amd import average, store
    _, _, texts = golden(w, o)
    frags = golden_fasta_path(tmp_path, w, o)
    out = str(tmp_path / "text")
    assert average.build(ctx, frags, out, out_fmt="text") == len(texts)
    got = _read_dir(out)
    assert sorted(got) == sorted(texts)
    for name in texts:
        assert got[name] == texts[name], name
    st, ref = str(tmp_path / "store"), str(tmp_path / "ref_store")
    average.build(ctx, frags, st, out_fmt="store")
    store.build_store(out, ref, np.float64)
    a, b = store.ProfileStore(st), store.ProfileStore(ref)
    assert a.ids == b.ids and a.letters == b.letters and a.lengths.tolist() == b.lengths.tolist() and a.n_pos == b.n_pos
    assert a.dtype == b.dtype
    assert np.array_equal(np.asarray(a.profile).view(np.int64), np.asarray(b.profile).view(np.int64))
    st32, ref32 = str(tmp_path / "store32"), str(tmp_path / "ref_store32")
    average.build(ctx, frags, st32, out_fmt="store", dtype=np.float32)
    store.build_store(out, ref32, np.float32)
    assert np.array_equal(np.asarray(store.ProfileStore(st32).profile).view(np.int32),
                          np.asarray(store.ProfileStore(ref32).profile).view(np.int32))


def test_fragments_command_reproduces_the_golden_windows(tmp_path):
    for w, o in PAIRS:
        seqs, frags, _ = golden(w, o)
        path = golden_fasta_path(tmp_path, w, o, "seqs")
        r = subprocess.run([sys.executable, "-m", "rnascan_amd.average", "fragments", path, "-w", str(w), "-o", str(o)],
                           cwd=REPO, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.split("\n")[:-1]
        got = [(lines[k][1:], lines[k + 1]) for k in range(0, len(lines), 2)]
        seq = dict(seqs)
        want = [("%s_frag_%d" % (rid, i), s[max(i, 0):i + w]) for rid, s in seqs if len(s) > 50 for i in py2_starts(len(s), w, o)]
        assert got == want
        names = {n for n, _ in got}
        for name, struct in frags:                       # the golden fragments are among them, their slices fit the structures
            assert name in names
            key, i = split_name(name)
            assert len(seq[key][max(i, 0):i + w]) == len(struct)


# ---- 2. random fragment sets against the restatement -----------------------------------------------------------------
def _random_set(rng, n_rec, tile_edges=True):
    """records [(id, [(start, structure)])] with negative starts, fragment lengths 1..300 and every position covered"""
    recs = []
    for r in range(n_rec):
        if tile_edges and r % 3 == 0:
            L = int(rng.choice([1, 63, 64, 65, 127, 128, 129, 255, 256, 257]))
        else:
            L = int(rng.integers(1, 900))
        frags = []
        at = 0
        while at < L:                                     # a chain of fragments that covers every position
            i = -int(rng.integers(0, 40)) if at == 0 else at - int(rng.integers(0, min(at, 50) + 1))
            p = max(i, 0)
            n = min(int(rng.integers(at - p + 1, at - p + 301)), L - p)
            frags.append((i, n))
            at = p + n
        for _ in range(int(rng.integers(0, 25))):          # and random others
            i = int(rng.integers(-150, L))
            n = min(int(rng.integers(1, 301)), L - max(i, 0))
            if n > 0:
                frags.append((i, n))
        order = rng.permutation(len(frags))               # starts in any order within a record
        recs.append(("rec%03d" % r, [(frags[k][0], random_structure(rng, frags[k][1])) for k in order]))
    return recs


def _write_frags(path, recs):
    with open(path, "w") as f:
        for rid, frags in recs:
            for i, s in frags:
                f.write(">%s_frag_%d some words\n" % (rid, i))
                for a in range(0, len(s), 60):
                    f.write(s[a:a + 60] + "\n")


def _want_rows(recs, dtype):
    rows = []
    for _, frags in recs:
        c = counts([max(i, 0) for i, _ in frags], [annotate(s) for _, s in frags])
        rows.append(scanned(c))
        rows.append(np.zeros((1, 7)))
    return np.concatenate(rows).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_sets_equal_the_restatement(ctx, tmp_path, dtype):
    from rnascan_amd import average
    rng = np.random.default_rng(11 if dtype == np.float64 else 12)
    recs = _random_set(rng, 60)
    # a record covered 1024 times, and one whose rows are covered 1 .. 300 times
    recs.append(("deep", [(int(i), random_structure(rng, 9)) for i in rng.integers(-3, 1, size=1024)]))
    recs.append(("ramp", [(k, random_structure(rng, 300 - k)) for k in range(300)]))
    path = str(tmp_path / "frags.fa")
    _write_frags(path, recs)
    fr = average.Fragments(path)
    assert fr.ids == [r for r, _ in recs]
    want = _want_rows(recs, dtype)
    rows, _ = average.average_batch(ctx, fr, 0, len(fr.ids), dtype=dtype)
    assert rows.dtype == dtype and rows.shape == want.shape
    assert np.array_equal(rows.view(np.uint8), want.view(np.uint8))
    # batches of a few records give the same rows
    parts = [average.average_batch(ctx, fr, a, b, dtype=dtype)[0] for a, b in fr.batches(letters=3000)]
    assert len(parts) > 5 and np.array_equal(np.concatenate(parts).view(np.uint8), want.view(np.uint8))


@pytest.mark.timeout(900)
def test_stream_longer_than_2_31(ctx):
    """two records, fragments of one 1000-letter structure at every start (coverage 1000): 2.2 x 10^9 fragment letters"""
    from rnascan_amd import _lib, average, dotbracket
    rng = np.random.default_rng(3)
    S = random_structure(rng, 1000)
    ann = np.array([COLUMNS.index(ch) for ch in annotate(S)], dtype=np.int64)
    unit = np.append(dotbracket.LUT[np.frombuffer(S.encode(), dtype=np.uint8)], np.uint8(7))
    F = [1_100_000, 1_100_000]
    L = [f + 999 for f in F]
    codes = np.tile(unit, sum(F))
    assert codes.size > (1 << 31)
    frag_off = np.arange(sum(F), dtype=np.int64) * 1001
    frag_len = np.full(sum(F), 1000, dtype=np.int64)
    rec_row = np.array([0, L[0] + 1], dtype=np.int64)
    frag_row = np.concatenate([np.arange(F[0]), rec_row[1] + np.arange(F[1])]).astype(np.int64)
    rec_frag = np.array([0, F[0], sum(F)], dtype=np.int64)
    T = average.value_table(1000)
    rows = ctx.average_host(codes, frag_off, frag_len, frag_row, rec_row, np.array(L), rec_frag, T, 1000, np.float64)
    del codes
    assert rows.shape == (sum(L) + 2, 7)
    for r in range(2):
        sample = np.concatenate([np.arange(1500), rng.integers(0, L[r], size=3000), np.arange(L[r] - 1500, L[r])])
        for p in sample.tolist():
            s = np.arange(max(0, p - 999), min(p, F[r] - 1) + 1)
            c = np.bincount(ann[p - s], minlength=7)
            want = T[len(s) * (len(s) + 1) // 2 + c]
            assert np.array_equal(rows[rec_row[r] + p], want), (r, p)
        assert not rows[rec_row[r] + L[r]].any()
    assert _lib.MAX_COVER == 1024


# ---- 3. rejections ----------------------------------------------------------------------------------------------------
def _build_error(ctx, tmp_path, text, out_fmt="store"):
    from rnascan_amd import average
    p = tmp_path / "bad.fa"
    p.write_text(text)
    with pytest.raises(average.AverageError) as e:
        average.build(ctx, str(p), str(tmp_path / "out"), out_fmt=out_fmt)
    assert str(p) in str(e.value)
    return str(e.value)


def test_rejections_name_what_is_wrong(ctx, tmp_path):
    msg = _build_error(ctx, tmp_path, ">a_frag_0\n((..))\n>b_frag_0\n...\n>b_frag_5\n..\n")
    assert "position 4 of record 'b'" in msg and "no fragment" in msg
    msg = _build_error(ctx, tmp_path, ">a_frag_0\n...\n" + "".join(">c_frag_0\n(.)\n" for _ in range(1025)))
    assert "record 'c'" in msg and "1024" in msg
    msg = _build_error(ctx, tmp_path, ">a_frag_0\n...\n>b_frag_0\n..\n>a_frag_1\n..\n")
    assert "'a'" in msg and "contiguous" in msg
    msg = _build_error(ctx, tmp_path, ">a_frag_0\n...\n>a_frag_1x\n..\n")
    assert "a_frag_1x" in msg
    msg = _build_error(ctx, tmp_path, ">a_frag_0\n...\n>a_frag_1\n.((.)\n")
    assert "a_frag_1" in msg and "dot-bracket" in msg
    # the context still works after each of them
    from rnascan_amd import average
    p = tmp_path / "good.fa"
    p.write_text(">a_frag_-1\n(.)\n>a_frag_1\n....\n")
    fr = average.Fragments(str(p))
    rows, _ = average.average_batch(ctx, fr, 0, 1)
    assert rows.shape == (6, 7)


def test_ids_with_a_slash_are_refused_for_text(ctx, tmp_path):
    msg = _build_error(ctx, tmp_path, ">a/b_frag_0\n...\n", "text")
    assert "a/b" in msg


# ---- 4. staged rows ---------------------------------------------------------------------------------------------------
def test_staged_rows_scan_as_host_rows(ctx, tmp_path):
    from rnascan_amd import average
    rng = np.random.default_rng(5)
    recs = _random_set(rng, 40, tile_edges=False)
    path = str(tmp_path / "frags.fa")
    _write_frags(path, recs)
    fr = average.Fragments(path)
    rows, _ = average.average_batch(ctx, fr, 0, len(fr.ids))
    mo = ctx.motif(None, rng.normal(0, 1, size=(10, 7)))
    want = ctx.hits_host(mo, None, rows, thr_struct=-2.0)
    average.average_batch(ctx, fr, 0, len(fr.ids), stage=True)
    got = ctx.hits_staged(mo, thr_struct=-2.0)
    mo.close()
    assert len(want[0]) > 10
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


# ---- 5. the command line -----------------------------------------------------------------------------------------------
def _rnafold_text(frags, seq_of):
    out = []
    for name, s in frags:
        key, i = split_name(name)
        sl = seq_of[key][max(i, 0):max(i, 0) + len(s)]
        out.append(">%s\n%s\n%s ( -1.00)\n%s [ -1.20]\n%s { -0.90 d=2.00}\n frequency of mfe structure in ensemble 0.1; "
                   "ensemble diversity 2.00\n" % (name, sl, s, s, s))
    return "".join(out)


def _cli_files(tmp_path, ctx, w=100, o=95):
    from rnascan_amd import average
    seqs, frags, texts = golden(w, o)
    fa = golden_fasta_path(tmp_path, w, o)
    have = {split_name(n)[0] for n, _ in frags}
    seq_of = dict(seqs)
    sq = str(tmp_path / "seqs.fa")
    with open(sq, "w") as f:
        for rid, s in seqs:
            if rid in have:
                f.write(">%s\n%s\n" % (rid, s))
    rf = str(tmp_path / "frags.rnafold")
    with open(rf, "w") as f:
        f.write(_rnafold_text(frags, seq_of))
    tdir, sdir = str(tmp_path / "avgdir"), str(tmp_path / "avgstore")
    average.build(ctx, fa, tdir, out_fmt="text")
    average.build(ctx, fa, sdir, out_fmt="store")
    return fa, rf, sq, tdir, sdir


def _run(argv, engine):
    from rnascan_amd import cli
    out = io.StringIO()
    cli.main(argv, engine=engine, out=out)
    return out.getvalue()


def _rows_without_id(t):
    return sorted("\t".join(l.split("\t")[:-1]) for l in t.split("\n")[1:] if l)


def _same_as_directory_scan(got, want):
    """a scan of the text directory against the scan of the store: the same rows (a directory is read in glob order),
    scores within the 1e-6 that the directory and store scan paths keep between them (test_gpu_cli.test_profile_store_on_gpu)"""
    g, w = _rows_without_id(got), _rows_without_id(want)
    assert len(g) == len(w)
    for a, b in zip(g, w):
        a, b = a.split("\t"), b.split("\t")
        assert a[:-1] == b[:-1] and abs(float(a[-1]) - float(b[-1])) <= 1e-6, (a, b)


def test_cli_fragments_equal_the_built_profiles(engine, tmp_path):
    fa, rf, sq, tdir, sdir = _cli_files(tmp_path, engine.ctx)
    bg = tmp_path / "bg.txt"
    bg.write_text(repr({l: 1.0 / 7 for l in "EHTBLRM"}))
    for argv in (["-q", STRUCT_PFM, "-u", "-m", " -inf"], ["-q", STRUCT_PFM, "-B", str(bg), "-C", "0.01", "-m", "-4"],
                 ["-q", STRUCT_PFM, "-u", "-m", " -inf", "--profile-dtype", "float32"]):
        want = _run(argv + [sdir], engine)
        assert want.count("\n") > (1000 if "-inf" in argv[-1] + " ".join(argv) else 0)
        assert _run(argv + ["--struct-format", "fragments", fa], engine) == want
        assert _run(argv + ["--struct-format", "fragments-rnafold", rf], engine) == want
        if "float32" not in argv:                        # a directory's float32 rows are cast per batch, a store's per file
            _same_as_directory_scan(_run(argv + [tdir], engine), want)
    for argv in (["-p", SEQ_PFM, "-q", STRUCT_PFM, "-u", "-m", "-6"], ["-p", SEQ_PFM, "-q", STRUCT_PFM, "-u", "-m", " -inf"]):
        want = _run(argv + [sq, sdir], engine)
        assert want.count("\n") > (1000 if "-inf" in " ".join(argv) else 0)
        _same_as_directory_scan(_run(argv + [sq, tdir], engine), want)
        assert _run(argv + ["--struct-format", "fragments", sq, fa], engine) == want
        assert _run(argv + ["--struct-format", "fragments-rnafold", sq, rf], engine) == want


def test_cli_fragments_usage_and_rejection(tmp_path):
    from rnascan_amd import cli
    with pytest.raises(SystemExit):
        cli.getoptions(["-q", STRUCT_PFM, "-t", "((..))", "--struct-format", "fragments"])
    bad = tmp_path / "bad.fa"
    bad.write_text(">a_frag_0\n...\n>b_frag_0\n..\n>a_frag_1\n..\n")
    before = set(os.listdir(str(tmp_path)))
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "rnascan"), "-q", STRUCT_PFM, "-u", "--struct-format",
                        "fragments", str(bad)], capture_output=True, text=True, timeout=280, env=env)
    assert r.returncode != 0 and r.stdout == "" and "'a'" in r.stderr and str(bad) in r.stderr
    assert set(os.listdir(str(tmp_path))) == before                  # no temporary store left behind


def _clean_env(**extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra)
    return env


@pytest.mark.timeout(600)
def test_rnascan_gpus_2_on_fragments(engine, tmp_path):
    fa, _, sq, _, sdir = _cli_files(tmp_path, engine.ctx)
    tmp = tmp_path / "tmp"
    tmp.mkdir()
    cmd = [sys.executable, os.path.join(REPO, "bin", "rnascan"), "-p", SEQ_PFM, "-q", STRUCT_PFM, "-u", "-m", " -inf"]
    one = subprocess.run(cmd + [sq, sdir], env=_clean_env(), capture_output=True, text=True, timeout=280)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run(cmd + ["--gpus", "2", "--struct-format", "fragments", sq, fa],
                         env=_clean_env(RNASCAN_ONE_DEVICE="1", TMPDIR=str(tmp)), capture_output=True, text=True, timeout=280)
    assert two.returncode == 0, two.stderr[-3000:]
    assert one.stdout.count("\n") > 20 and two.stdout == one.stdout
    assert os.listdir(str(tmp)) == []
