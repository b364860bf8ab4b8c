"""Dot-bracket structure input on the device: the annotation kernels (csrc/pfmscan_dotbracket.hip) against the reference
parser's output (tests/golden/dotbracket/) and the restatement of its rules (tests/dotbracket_rules.py), rejection of
invalid records, and every structure-letter mode of the CLI on dot-bracket files against the same run on the letters."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA_DIR, REPO
from dotbracket_rules import annotate, count_letters, deep_structure, random_structure
from test_dotbracket_cpu import load_fixtures

pytestmark = pytest.mark.gpu

SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")
LETTERS = "EHTBLRM"


@pytest.fixture(scope="module")
def engine():
    from rnascan_amd import scanner
    e = scanner.HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(engine):
    return engine.ctx


def _pack(structs):
    from rnascan_amd import dotbracket, pack
    return pack.pack([dotbracket.LUT[np.frombuffer(s.encode("latin-1"), dtype=np.uint8)] for s in structs])


def _letters_of(codes, s):
    """annotated codes of a packed stream -> one string per record"""
    return [bytes(np.frombuffer(LETTERS.encode(), dtype=np.uint8)[codes[o:o + n]]).decode() if n else ""
            for o, n in zip(s.offsets.tolist(), s.lengths.tolist())]


def _check_stream(got, s, want_strings):
    from rnascan_amd import pack
    seps = s.offsets + s.lengths
    assert np.all(got[seps] == pack.SEP)
    assert got.max(initial=0) <= pack.SEP
    assert _letters_of(got, s) == want_strings


def _staged_codes(ctx, n):
    """the codes staged in ctx, read back through a width-1 letter scan whose score is the letter's code"""
    T = np.full((1, 8), np.nan)
    T[0, :7] = np.arange(7)
    mo = ctx.motif(T, None)
    pos, sc = ctx.hits_letters_f64_staged(mo, -np.inf)
    mo.close()
    out = np.full(n, 7, dtype=np.uint8)
    out[pos] = sc.astype(np.uint8)
    return out


# ---- 1. the device equals the reference --------------------------------------------------------------------------------
def test_dev_staged_host_equal_the_reference(ctx):
    import torch
    structs, ref = load_fixtures()
    s = _pack(structs)
    want_counts = count_letters("".join(ref))
    got, counts = ctx.dotbracket_annotate_host(s.codes)
    _check_stream(got, s, ref)
    assert np.array_equal(counts, want_counts)
    # staged: in the codes slot, read back by a scan
    c2 = ctx.dotbracket_stage(s.codes)
    assert np.array_equal(c2, want_counts)
    assert np.array_equal(_staged_codes(ctx, s.n_pos), got)
    # device buffers (torch's allocator), histogram on the device
    d_in = torch.from_numpy(s.codes).to("cuda:0")
    d_out = torch.empty_like(d_in)
    d_counts = torch.full((7,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.dotbracket_annotate_dev(d_in, d_out, s.n_pos, d_counts=d_counts)
    ctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), got)
    assert np.array_equal(d_counts.cpu().numpy(), want_counts)


def test_letter_map_is_the_callers(ctx):
    structs, ref = load_fixtures()
    s = _pack(structs[:300])
    perm = np.array([6, 0, 5, 1, 4, 2, 3], dtype=np.uint8)
    got, counts = ctx.dotbracket_annotate_host(s.codes, letter_map=perm)
    base, base_counts = ctx.dotbracket_annotate_host(s.codes)
    lut = np.append(perm, np.uint8(7))
    assert np.array_equal(got, lut[base])
    assert np.array_equal(counts[perm], base_counts)
    with pytest.raises(ValueError):
        ctx.dotbracket_annotate_host(s.codes, letter_map=np.array([0, 1, 2, 3, 4, 5, 7]))


# ---- 2. random structures equal the restatement ----------------------------------------------------------------------
def test_random_structures_equal_the_restatement(ctx):
    rng = np.random.default_rng(123)
    structs = ["", ".", "(", ")", "()", "..", "((", "(((())))", "()()()", "......", "((()))(())"]
    structs = [x for x in structs if x.count("(") == x.count(")") and x.find(")") >= x.find("(")]
    structs += ["", "", ".", "()"] * 5
    for _ in range(1500):
        n = int(np.exp(rng.uniform(0, np.log(6000))))
        structs.append(random_structure(rng, n))
    structs += ["." * 9000, "(" * 4500 + ")" * 4500, "()" * 5000]          # all-dot, dot-free, across many tiles
    # stems that cross every tile boundary: one long record whose pairs span 1 .. 20 000 positions
    structs.append("".join("(" * 40 + random_structure(rng, int(rng.integers(1, 20000))) + ")" * 40 + "." * int(rng.integers(0, 50))
                           for _ in range(30)))
    s = _pack(structs)
    got, counts = ctx.dotbracket_annotate_host(s.codes)
    want = [annotate(x) for x in structs]
    _check_stream(got, s, want)
    assert np.array_equal(counts, count_letters("".join(want)))
    # the same records one tile boundary over: shift the stream by every offset of a small set
    for shift in (1, 15, 16, 63, 64, 4095):
        sh = _pack(["." * shift] + structs[-40:])
        g, _ = ctx.dotbracket_annotate_host(sh.codes)
        _check_stream(g, sh, ["E" * shift] + want[-40:])


def test_one_million_positions_depth_one_hundred_thousand(ctx):
    rng = np.random.default_rng(7)
    body = random_structure(rng, 1_000_000 - 200_000, 0.6)
    rec = "(" * 50_000 + "." + "(" * 50_000 + body + ")" * 50_000 + "." * 3 + ")" * 50_000
    assert len(rec) == 1_000_004
    s = _pack([rec, deep_structure(100_000), "."])
    got, _ = ctx.dotbracket_annotate_host(s.codes)
    _check_stream(got, s, [annotate(rec), annotate(deep_structure(100_000)), "E"])


# ---- 3. rejection --------------------------------------------------------------------------------------------------
BAD = [("extra (", lambda r: r[:3] + "(" + r[3:]), ("extra )", lambda r: r[:3] + ")" + r[3:]), ("[", lambda r: r[:5] + "[" + r[5:]),
       ("space", lambda r: r[:4] + " " + r[4:]), ("energy", lambda r: r + "-1.20")]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_rejection_names_the_record_and_leaves_the_ctx_usable(ctx, what, spoil):
    from rnascan_amd import dotbracket
    rng = np.random.default_rng(3)
    structs = [random_structure(rng, int(rng.integers(10, 3000))) for _ in range(50)]
    k = 31
    bad = list(structs)
    bad[k] = spoil("((...))" + bad[k])
    s = _pack(bad)
    with pytest.raises(ValueError) as ei:
        ctx.dotbracket_annotate_host(s.codes)
    pos = ei.value.position
    assert dotbracket.record_of(s.offsets, pos) == k
    with pytest.raises(ValueError) as ei:
        ctx.dotbracket_stage(s.codes)
    assert dotbracket.record_of(s.offsets, ei.value.position) == k
    assert int(ctx._L.pfmscan_staged_positions(ctx._h)) == -1            # nothing staged after a rejected stream
    # the same ctx then annotates and scans a valid stream
    good = _pack(structs)
    got, _ = ctx.dotbracket_annotate_host(good.codes)
    _check_stream(got, good, [annotate(x) for x in structs])
    ctx.dotbracket_stage(good.codes)
    assert np.array_equal(_staged_codes(ctx, good.n_pos), got)


def test_stream_without_a_final_separator_is_rejected(ctx):
    s = _pack(["((..))"])
    with pytest.raises(ValueError) as ei:
        ctx.dotbracket_annotate_host(s.codes[:-1])
    assert ei.value.position == s.n_pos - 2
    got, counts = ctx.dotbracket_annotate_host(np.zeros(0, dtype=np.uint8))
    assert got.size == 0 and counts.sum() == 0


# ---- 4. the CLI on dot-bracket files equals the CLI on their letters ---------------------------------------------------
def _files(tmp_path, n=120, seed=17, with_seq=False):
    rng = np.random.default_rng(seed)
    structs = [random_structure(rng, int(rng.integers(0, 2500))) for _ in range(n)] + ["." * 40, "(" * 20 + ")" * 20, ""]
    db, lt, sq = tmp_path / "dot.fa", tmp_path / "letters.fa", tmp_path / "seqs.fa"
    with open(db, "w") as f, open(lt, "w") as g, open(sq, "w") as h:
        for i, x in enumerate(structs):
            f.write(">r%d some description (%d)\n" % (i, i))
            for a in range(0, len(x), 70):                               # wrapped lines in the dot-bracket file
                f.write(x[a:a + 70] + "\n")
            g.write(">r%d some description (%d)\n%s\n" % (i, i, annotate(x)))
            h.write(">r%d some description (%d)\n%s\n" % (i, i, "".join(rng.choice(list("ACGU"), size=len(x)))))
    return str(db), str(lt), str(sq)


def _run(argv, engine):
    from rnascan_amd import cli
    out = io.StringIO()
    cli.main(argv, engine=engine, out=out)
    return out.getvalue()


def _same(got, want, what):
    if got == want:
        return
    g, w = got.split("\n"), want.split("\n")
    for i in range(max(len(g), len(w))):
        a, b = (g[i] if i < len(g) else "<end>"), (w[i] if i < len(w) else "<end>")
        if a != b:
            raise AssertionError("%s: %d / %d lines, first difference at line %d:\n got  %s\n want %s" % (what, len(g), len(w), i, a, b))


def _struct_library(tmp_path, n=256, seed=4):
    from test_scanner_cpu import _write_multi_pfm
    rng = np.random.default_rng(seed)
    motifs = [("M%03d" % k, list(LETTERS), rng.dirichlet(np.full(7, 0.4), size=int(rng.choice([4, 6, 8, 12])))) for k in range(n)]
    path = str(tmp_path / "struct_lib.pfm")
    _write_multi_pfm(path, motifs)
    seq = [("M%03d" % k, list("ACGU"), rng.dirichlet(np.full(4, 0.5), size=len(M))) for k, (_, _, M) in enumerate(motifs[:40])]
    spath = str(tmp_path / "seq_lib.pfm")
    _write_multi_pfm(spath, seq)
    tpath = str(tmp_path / "struct_lib40.pfm")
    _write_multi_pfm(tpath, motifs[:40])
    return path, spath, tpath


def test_cli_dotbracket_equals_letters(engine, tmp_path):
    db, lt, sq = _files(tmp_path)
    bg = tmp_path / "bg.txt"
    bg.write_text(repr({l: 1.0 / 7 for l in LETTERS}))
    lib, seq_lib, lib40 = _struct_library(tmp_path)
    cases = [
        ["-q", STRUCT_PFM, "-m", "6"],
        ["-q", STRUCT_PFM, "-m", "1.5"],
        ["-q", STRUCT_PFM, "-m", " -inf"],
        ["-q", STRUCT_PFM, "-C", "0.01", "-m", "1"],
        ["-q", STRUCT_PFM, "-u", "-m", "2"],
        ["-q", STRUCT_PFM, "-B", str(bg), "-m", "2"],
        ["-q", lib, "-m", "4"],
    ]
    for argv in cases:
        want = _run(argv + [lt], engine)
        if "-inf" in "".join(argv):
            assert want.count("\n") > 1000
        _same(_run(argv + [db], engine), want, " ".join(argv))
        _same(_run(argv + ["--struct-format", "dotbracket", db], engine), want, " ".join(argv) + " (explicit)")
    # two-FASTA RNASS, and the two-FASTA library
    for argv in (["-p", SEQ_PFM, "-q", STRUCT_PFM, "-m", "0"], ["-p", seq_lib, "-q", lib40, "-m", "1"]):
        want = _run(argv + [sq, lt], engine)
        assert want.count("\n") > 1
        _same(_run(argv + [sq, db], engine), want, " ".join(argv))


def test_cli_bgonly_and_testseq(engine, tmp_path):
    from rnascan_amd import cli
    db, lt, _ = _files(tmp_path, n=40)
    outs = []
    for path in (lt, db):
        out = io.StringIO()
        with pytest.raises(SystemExit):
            cli.main(["-q", STRUCT_PFM, "-g", path], engine=engine, out=out)
        outs.append(out.getvalue())
    assert outs[0] == outs[1] and outs[0].startswith("{")
    s = "..((((...))))...((..((...))..))."
    _same(_run(["-q", STRUCT_PFM, "-m", " -inf", "-t", s], engine), _run(["-q", STRUCT_PFM, "-m", " -inf", "-t", annotate(s)], engine),
          "-t struct")
    both = "ACGUACGUACGUACGUACGUACGUACGUACGU," + s
    _same(_run(["-p", SEQ_PFM, "-q", STRUCT_PFM, "-m", " -inf", "-t", both], engine),
          _run(["-p", SEQ_PFM, "-q", STRUCT_PFM, "-m", " -inf", "-t", both.split(",")[0] + "," + annotate(s)], engine), "-t seq,struct")


def test_cli_letters_format_is_todays_behaviour(engine, tmp_path):
    """--struct-format letters on a dot-bracket file: every window holds a foreign letter, as before this option"""
    db, _, _ = _files(tmp_path, n=30)
    foreign = tmp_path / "foreign.fa"
    from rnascan_amd import fasta
    with open(foreign, "w") as f:
        for rec in fasta.parse_sequences(db):
            f.write(">%s\n%s\n" % (rec.description, "X" * len(rec.seq)))
    for argv in (["-q", STRUCT_PFM, "-m", " -inf", "-u"], ["-q", STRUCT_PFM, "-m", "0", "-u"]):
        _same(_run(argv + ["--struct-format", "letters", db], engine), _run(argv + [str(foreign)], engine), " ".join(argv))


def test_cli_rejects_an_invalid_record(tmp_path):
    rng = np.random.default_rng(8)
    fa = tmp_path / "bad.fa"
    with open(fa, "w") as f:
        for i in range(20):
            x = random_structure(rng, int(rng.integers(5, 500)))
            if i == 13:
                x = "((..)).. (-1.20)"
            f.write(">rec%d\n%s\n" % (i, x))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bin", "rnascan"), "-q", STRUCT_PFM, str(fa)],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode != 0 and r.stdout == ""
    assert "rec13" in r.stderr and str(fa) in r.stderr
    r = subprocess.run([sys.executable, "-m", "rnascan_amd.dotbracket", str(fa)], cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode != 0 and r.stdout == "" and "rec13" in r.stderr


# ---- 5. --gpus 2 rehearsed on one GPU; 6. the converter ------------------------------------------------------------------
def _clean_env(**extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra)
    return env


@pytest.mark.timeout(600)
def test_rnascan_gpus_2_equals_one_rank_on_dotbracket(tmp_path):
    db, lt, _ = _files(tmp_path, n=300, seed=21)
    cmd = [sys.executable, os.path.join(REPO, "bin", "rnascan"), "-q", STRUCT_PFM, "-C", "0.01", "-m", "1"]
    one = subprocess.run(cmd + [lt], env=_clean_env(), capture_output=True, text=True, timeout=280)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run(cmd + ["--gpus", "2", db], env=_clean_env(RNASCAN_ONE_DEVICE="1"), capture_output=True, text=True, timeout=280)
    assert two.returncode == 0, two.stderr[-3000:]
    assert one.stdout.count("\n") > 50
    assert two.stdout == one.stdout


def test_converter_writes_the_letters_file(tmp_path):
    db, lt, _ = _files(tmp_path, n=60, seed=5)
    r = subprocess.run([sys.executable, "-m", "rnascan_amd.dotbracket", db], cwd=REPO, capture_output=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(lt, "rb") as f:
        assert r.stdout == f.read()


# ---- 7. full size ----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_c3_size_is_deterministic_and_right(ctx):
    """100 000 records of 3 kb (C3's size): each one a random 100-position head and one of 16 random 2 900-position
    bodies, so that no two neighbouring records need be alike"""
    from rnascan_amd import dotbracket
    rng = np.random.default_rng(100)
    n_rec, L, H = 100_000, 3000, 100
    heads = [random_structure(rng, H) for _ in range(256)]
    bodies = [random_structure(rng, L - H) for _ in range(16)]
    head_c = np.stack([dotbracket.LUT[np.frombuffer(x.encode(), dtype=np.uint8)] for x in heads])
    body_c = np.stack([dotbracket.LUT[np.frombuffer(x.encode(), dtype=np.uint8)] for x in bodies])
    hw, bw = rng.integers(0, 256, size=n_rec), rng.integers(0, 16, size=n_rec)
    view = np.full((n_rec, L + 1), 7, dtype=np.uint8)
    view[:, :H] = head_c[hw]
    view[:, H:L] = body_c[bw]
    codes = view.reshape(-1)
    a, ca = ctx.dotbracket_annotate_host(codes)
    b, cb = ctx.dotbracket_annotate_host(codes)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    assert int(ca.sum()) == n_rec * L
    a = a.reshape(n_rec, L + 1)
    assert np.all(a[:, L] == 7)
    for r in rng.choice(n_rec, size=200, replace=False):
        want = annotate(heads[hw[r]] + bodies[bw[r]])
        assert bytes(np.frombuffer(LETTERS.encode(), dtype=np.uint8)[a[r, :L]]).decode() == want, r


@pytest.mark.timeout(1200)
def test_stream_longer_than_2_31(ctx):
    """a stream of 2^31 + 6 million positions on one device: records around position 2^31 equal the restatement, the
    histogram equals a count of the output"""
    from rnascan_amd import _lib, dotbracket
    rng = np.random.default_rng(31)
    L = 2999
    pool = [random_structure(rng, L) for _ in range(32)]
    pool_c = np.stack([np.append(dotbracket.LUT[np.frombuffer(x.encode(), dtype=np.uint8)], np.uint8(7)) for x in pool])
    n_rec = (1 << 31) // (L + 1) + 2000
    pick = rng.integers(0, 32, size=n_rec)
    codes = pool_c[pick].reshape(-1)
    assert codes.size > (1 << 31) + 1_000_000
    out, counts = ctx.dotbracket_annotate_host(codes)
    del codes
    assert np.array_equal(counts, _lib.count_bytes(out)[:7])
    cut = (1 << 31) // (L + 1)
    assert cut * (L + 1) < (1 << 31) < (cut + 1) * (L + 1)
    for r in list(range(cut - 3, cut + 4)) + [n_rec - 1]:              # the records around position 2^31, and the last
        got = out[r * (L + 1):(r + 1) * (L + 1)]
        assert got[L] == 7
        assert bytes(np.frombuffer(LETTERS.encode(), dtype=np.uint8)[got[:L]]).decode() == annotate(pool[pick[r]]), r
